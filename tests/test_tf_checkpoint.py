"""Row f-2: TensorFlow checkpoint reader.  The two `.index` files under tests/golden/tf_ckpt are DATA files
shipped by the reference (model/2000pickle_base, 1.8 KB and 8.7 KB).  The 1.2 MB weight shards are not part of this
repository: the loading tests write actor checkpoints of their own in the published layout instead (every entry, offset
and size of the published actor index; seeded weights; the CRC-32Cs of those weights), see `_write_actor_checkpoint`."""
import os
import struct

import numpy as np
import pytest
import torch

import tf_checkpoint as T

FX = os.path.join(os.path.dirname(__file__), "golden", "tf_ckpt")
PUBLISHED_ACTOR = os.path.join(FX, "Agent1_Actor_pickle")


def _pb_varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _pb_encode(fields):
    """T._fields(...) -> protobuf wire bytes"""
    out = bytearray()
    for fn, wt, v in fields:
        out += _pb_varint(fn << 3 | wt)
        if wt == 0:
            out += _pb_varint(v)
        elif wt == 2:
            out += _pb_varint(len(v)) + bytes(v)
        else:                                             # fixed64 / fixed32: raw bytes
            out += bytes(v)
    return bytes(out)


def _table_block(entries):
    """one uncompressed table block (no key sharing, one restart point) + its 5-byte trailer"""
    blk = bytearray()
    for k, v in entries:
        blk += _pb_varint(0) + _pb_varint(len(k)) + _pb_varint(len(v)) + k + v
    blk += struct.pack("<II", 0, 1)
    return bytes(blk), b"\0" + struct.pack("<I", T.masked_crc32c(bytes(blk) + b"\0"))


def _write_actor_checkpoint(prefix, seed):
    """`<prefix>.index` + `<prefix>.data-00000-of-00001`: the published actor's entries (names, dtypes, shapes, offsets,
    sizes, header) read from its `.index`, filled with seeded weights (non-weight entries: seeded bytes), every entry's
    CRC-32C recomputed; the index is written as one data block + empty metaindex + index block + footer, as TensorFlow
    writes it.  Returns {variable name: array} of what was written."""
    data = open(PUBLISHED_ACTOR + ".index", "rb").read()
    footer = data[-48:]
    _, _, p = T._handle(footer, 0)
    ioff, isize, _ = T._handle(footer, p)
    raw = [kv for _, hv in T._block(data, ioff, isize) for kv in T._block(data, *T._handle(hv, 0)[:2])]
    idx = T.read_index(PUBLISHED_ACTOR + ".index")
    rng = np.random.default_rng(seed)
    blob = bytearray(max(e["offset"] + e["size"] for e in idx.values()))
    written, entries = {}, []
    for key, val in raw:
        name = key.decode()
        if name:
            e = idx[name]
            if e["dtype"] == 1 and name.startswith("gcn_"):
                arr = (rng.standard_normal(e["shape"]) * 0.05).astype(np.float32)
                written[name[: -len("/.ATTRIBUTES/VARIABLE_VALUE")]] = arr
                chunk = arr.tobytes()
            else:
                chunk = rng.integers(0, 256, e["size"], dtype=np.uint8).tobytes()
            assert len(chunk) == e["size"]
            blob[e["offset"]:e["offset"] + e["size"]] = chunk
            val = _pb_encode([(fn, wt, struct.pack("<I", T.masked_crc32c(chunk)) if fn == 6 else v)
                              for fn, wt, v in T._fields(val)])
        entries.append((key, val))
    blk, trailer = _table_block(entries)
    meta, meta_trailer = _table_block([])
    ix, ix_trailer = _table_block([(b"p", _pb_varint(0) + _pb_varint(len(blk)))])    # key: a separator after the last key
    out = blk + trailer
    meta_h = _pb_varint(len(out)) + _pb_varint(len(meta))
    out += meta + meta_trailer
    ix_h = _pb_varint(len(out)) + _pb_varint(len(ix))
    out += ix + ix_trailer
    handles = meta_h + ix_h
    out += handles + b"\0" * (40 - len(handles)) + struct.pack("<Q", 0xDB4775248B80FB57)
    open(prefix + ".index", "wb").write(out)
    open(prefix + ".data-00000-of-00001", "wb").write(bytes(blob))
    return written


@pytest.fixture(scope="module")
def actor_dir(tmp_path_factory):
    """Agent{1,2,3}_Actor_pickle checkpoints in the published layout (seeds 1-3) and the published critic index without
    its shard (not published), the directory layout of model/2000pickle_base."""
    d = tmp_path_factory.mktemp("2000pickle_base")
    weights = {a: _write_actor_checkpoint(str(d / f"Agent{a}_Actor_pickle"), a) for a in (1, 2, 3)}
    crit = open(os.path.join(FX, "Agent1_Critic_pickle.index"), "rb").read()
    (d / "Agent1_Critic_pickle.index").write_bytes(crit)
    return str(d), weights


def test_index_of_published_actor():
    idx = T.read_index(os.path.join(FX, "Agent1_Actor_pickle.index"))
    kern = {k: v for k, v in idx.items() if k.endswith("kernel/.ATTRIBUTES/VARIABLE_VALUE")}
    assert len(kern) == 13                                             # 13 GCN layers (truss2D_RL.py:49-120)
    assert idx["gcn_l1_1/kernel/.ATTRIBUTES/VARIABLE_VALUE"]["shape"] == (13, 200)
    assert idx["gcn_l1_4/kernel/.ATTRIBUTES/VARIABLE_VALUE"]["shape"] == (4, 200)
    assert idx["gcn_l4_1/kernel/.ATTRIBUTES/VARIABLE_VALUE"]["shape"] == (200, 2)
    assert idx["gcn_l4_2/kernel/.ATTRIBUTES/VARIABLE_VALUE"]["shape"] == (200, 3)
    n = sum(int(np.prod(v["shape"])) for k, v in idx.items() if k.startswith("gcn_"))
    assert n == 291805                                                 # 3x(13x200+200) + (4x200+200) + 7x(200x200+200) + (200x2+2) + (200x3+3)
    # offsets tile the data shard without overlap
    spans = sorted((v["offset"], v["offset"] + v["size"]) for v in idx.values() if v["size"])
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert "_CHECKPOINTABLE_OBJECT_GRAPH" in idx


def test_index_of_published_critic_lists_all_layers():
    idx = T.read_index(os.path.join(FX, "Agent1_Critic_pickle.index"))
    gcn = {k.split("/")[0] for k in idx if k.startswith("gcn_")}
    assert len(gcn) == 21 and {"dense_1", "dense_2"} <= {k.split("/")[0] for k in idx}      # 21 GCN + MLP


def test_bad_file_is_refused(tmp_path):
    p = tmp_path / "x.index"
    p.write_bytes(b"not a table" * 10)
    with pytest.raises(ValueError):
        T.read_index(str(p))


def test_crc32c_known_answers():
    assert T.crc32c(b"123456789") == 0xE3069283                       # CRC-32C check value
    assert T.crc32c(b"") == 0


def test_written_checkpoint_has_the_published_layout(actor_dir):
    """the fixture's index lists exactly the published entries (dtype, shape, shard, offset, size); only the CRCs differ"""
    d, _ = actor_dir
    pub = T.read_index(PUBLISHED_ACTOR + ".index")
    for a in (1, 2, 3):
        own = T.read_index(os.path.join(d, f"Agent{a}_Actor_pickle.index"))
        assert own.keys() == pub.keys()
        strip = lambda e: {k: v for k, v in e.items() if k != "crc32c"}
        assert all(strip(own[k]) == strip(pub[k]) for k in pub)


def test_published_actors_load_and_run(actor_dir):
    import truss2D_RL as RL
    d, weights = actor_dir
    for agent in (1, 2, 3):
        actor = RL.multimodes_actor(200, 2, 3)
        n = T.load_gcn_actor(actor, os.path.join(d, f"Agent{agent}_Actor_pickle"))     # CRC-checked
        assert n == 291805
        assert np.array_equal(actor.gcn_l1_1.lin.weight.detach().numpy(), weights[agent]["gcn_l1_1/kernel"].T)
        N, Pn = 16, 20
        g = torch.Generator().manual_seed(agent)
        A = torch.eye(N).unsqueeze(0)
        ins = (torch.rand(1, N, 13, generator=g), A, A, A, A, torch.rand(1, Pn, 4, generator=g), torch.eye(Pn).unsqueeze(0))
        with torch.no_grad():
            geo, topo = actor(ins)
        assert geo.shape == (1, N, 2) and topo.shape == (1, N, 3)
        assert torch.isfinite(geo).all() and (geo > 0).all() and (geo < 1).all() and (topo > 0).all() and (topo < 1).all()
        assert sum(p.numel() for p in actor.parameters()) == 291805
    # the critic shards are not shipped (model/.../.MISSING_LARGE_BLOBS): a clear error, not garbage
    with pytest.raises((ValueError, FileNotFoundError)):
        T.load_variables(os.path.join(d, "Agent1_Critic_pickle"))
    # a corrupted weight is refused by its CRC
    bad = os.path.join(d, "corrupt")
    _write_actor_checkpoint(bad, 9)
    blob = bytearray(open(bad + ".data-00000-of-00001", "rb").read())
    blob[5] ^= 1
    open(bad + ".data-00000-of-00001", "wb").write(bytes(blob))
    with pytest.raises(ValueError, match="CRC"):
        T.load_variables(bad)


def test_maddpg_restores_published_actors(actor_dir):
    import truss2D_RL as RL
    import master_DDPG_truss2D_MO as M
    d, weights = actor_dir
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, M.a_nn, M.c_nn, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cpu")
    rl.load_weights(d + "/")                        # the reference's own directory layout (master…:710-729)
    v = T.load_variables(os.path.join(d, "Agent2_Actor_pickle"), verify=False)
    w = rl.agents[1].actor_model.gcn_l2_3.lin.weight.detach().numpy()
    assert np.array_equal(w, v["gcn_l2_3/kernel"].T)
    assert np.array_equal(rl.agents[1].target_actor_model.gcn_l4_2.bias.detach().numpy(), v["gcn_l4_2/bias"])
    for a in (1, 2, 3):
        assert np.array_equal(rl.agents[a - 1].actor_model.gcn_l3_2.bias.detach().numpy(), weights[a]["gcn_l3_2/bias"])
