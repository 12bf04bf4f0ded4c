// truss_replay.h -- the replay buffer's two data movements, each ONE launch for every field of a transition (gfx950):
//   truss_replay_scatter  append: ring row (head + r) % capacity of every field <- row rows[group][r] of the tensor outside the ring
//   truss_replay_gather   sample: row r of every output <- ring row idx[r]
// (include/truss_mi355.h).  A field is `plain` (a row of parts x part_len floats; the outside tensor may be strided in two levels) or
// `pattern` (a dense [n][n] matrix outside, [n][k_nbr] inside the ring, through the neighbour table).  Nothing is computed: values
// travel as 32-bit words, so every bit pattern survives.  Fields are slices of the grid (grid.y, descriptors by value in the kernel
// arguments as in truss_gcn_level.h); within a field a thread moves one PIECE of a row -- four consecutive floats -- per iteration of
// a grid-stride loop, as one 16-byte access where both addresses are 16-byte aligned and the piece is whole, word by word otherwise
// (a 13-float part: three whole pieces and a one-word tail; a 4-byte aligned view: words).  No LDS, no atomics: every output word
// has one owner.  Row indices come from device memory and are range-checked by the thread that uses them (a bad index skips the row).
#pragma once

#define TRP_MAX 32               // fields per launch (32 x 80 bytes of kernel arguments)
#define TRP_BLOCKS 1024          // workgroups per field at most; the grid-stride loop covers the rest

struct ReplayFieldDev {
  uint32_t *ring, *ext;
  const int16_t *nbr;
  long ext_rows, ext_row_stride, ext_part_stride;
  int part_len, n, k_nbr, group;
  int ring_row;                  // words per ring row
  unsigned pp;                   // plain: pieces per part
  unsigned per_row;              // pieces per row
  unsigned nblocks;              // workgroups this field uses
};
struct ReplayDev {
  ReplayFieldDev f[TRP_MAX];
  const long long *rows;         // scatter: [4][k] source rows; gather: [k] ring rows
  long head, capacity;
  int k;
};

__device__ __forceinline__ void trp_store(uint32_t *d, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, int cnt) {
  if (cnt == 4 && ((size_t)d & 15) == 0) {
    *(uint4 *)d = make_uint4(v0, v1, v2, v3);
  } else {
    d[0] = v0;
    if (cnt > 1) d[1] = v1;
    if (cnt > 2) d[2] = v2;
    if (cnt > 3) d[3] = v3;
  }
}

template <bool GATHER>
__global__ __launch_bounds__(256) void truss_replay_kernel(const ReplayDev D) {
  const ReplayFieldDev &F = D.f[blockIdx.y];
  if (blockIdx.x >= F.nblocks) return;
  const unsigned total = (unsigned)D.k * F.per_row;                  // (< 2^31: checked by the host)
  const unsigned stride = F.nblocks * 256u;
  for (unsigned w = blockIdx.x * 256u + threadIdx.x; w < total; w += stride) {
    const unsigned r = w / F.per_row, q = w - r * F.per_row;
    long ring_row, ext_row;
    if (GATHER) {
      ring_row = D.rows[r];
      ext_row = r;
      if ((unsigned long)ring_row >= (unsigned long)D.capacity) continue;
    } else {
      ring_row = D.head + r;
      if (ring_row >= D.capacity) ring_row -= D.capacity;
      ext_row = D.rows[(long)F.group * D.k + r];
      if ((unsigned long)ext_row >= (unsigned long)F.ext_rows) continue;
    }
    uint32_t *ring = F.ring + ring_row * F.ring_row;
    uint32_t *ext = F.ext + ext_row * F.ext_row_stride;
    if (!F.nbr) {
      // ---- plain: piece q of the row = words [off, off + cnt) of part `part` ----
      const unsigned part = q / F.pp, off = (q - part * F.pp) * 4u;
      const int cnt = F.part_len - (int)off < 4 ? F.part_len - (int)off : 4;
      uint32_t *rp = ring + (long)part * F.part_len + off;
      uint32_t *ep = ext + (long)part * F.ext_part_stride + off;
      const uint32_t *s = GATHER ? rp : ep;
      uint32_t *d = GATHER ? ep : rp;
      if (cnt == 4 && (((size_t)s | (size_t)d) & 15) == 0) {
        *(uint4 *)d = *(const uint4 *)s;
      } else {
        for (int j = 0; j < cnt; ++j) d[j] = s[j];
      }
    } else if (!GATHER) {
      // ---- pattern, append: words [e0, e0 + cnt) of the compact row [n][k_nbr] <- the dense matrix at the listed columns ----
      const int n = F.n, kn = F.k_nbr, nk = n * kn, e0 = (int)q * 4;
      const int cnt = nk - e0 < 4 ? nk - e0 : 4;
      uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
          const int e = e0 + j, i = e / kn, c = F.nbr[e];
          if (c >= 0 && c < n) v[j] = ext[(long)i * n + c];
        }
      }
      trp_store(ring + e0, v[0], v[1], v[2], v[3], cnt);
    } else {
      // ---- pattern, sample: words [e0, e0 + cnt) of the dense matrix <- zeros, then the listed entries of the compact row ----
      const int n = F.n, kn = F.k_nbr, nn = n * n, e0 = (int)q * 4;
      const int cnt = nn - e0 < 4 ? nn - e0 : 4;
      uint32_t v0 = 0u, v1 = 0u, v2 = 0u, v3 = 0u;
      if ((n & 3) == 0) {                                              // the four columns [c0, c0 + 4) of one matrix row: one pass over its slots
        const int i = e0 / n, c0 = e0 - i * n;
        for (int s = 0; s < kn; ++s) {
          const unsigned dlt = (unsigned)((int)F.nbr[i * kn + s] - c0);
          if (dlt < 4u) {
            const uint32_t val = ring[i * kn + s];
            v0 = dlt == 0u ? val : v0;
            v1 = dlt == 1u ? val : v1;
            v2 = dlt == 2u ? val : v2;
            v3 = dlt == 3u ? val : v3;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < cnt) {
            const int e = e0 + j, i = e / n, col = e - i * n;
            uint32_t val = 0u;
            for (int s = 0; s < kn; ++s)
              if ((int)F.nbr[i * kn + s] == col) val = ring[i * kn + s];
            v0 = j == 0 ? val : v0;
            v1 = j == 1 ? val : v1;
            v2 = j == 2 ? val : v2;
            v3 = j == 3 ? val : v3;
          }
        }
      }
      trp_store(ext + e0, v0, v1, v2, v3, cnt);
    }
  }
}

static int trp_run(const char *what, bool gather, const truss_replay_field_t *fields, int32_t n_fields, const int64_t *rows, int32_t k,
                   int64_t head, int64_t capacity, void *stream) {
  const std::string me(what);
  if (n_fields < 0 || k < 0) return tb_fail(TRUSS_EINVAL, me + ": negative count");
  if (capacity < 1) return tb_fail(TRUSS_EINVAL, me + ": capacity < 1");
  if (!gather && (head < 0 || head >= capacity || k > capacity)) return tb_fail(TRUSS_EINVAL, me + ": head outside [0, capacity) or k > capacity");
  if (n_fields == 0 || k == 0) return TRUSS_OK;
  if (!fields || !rows) return tb_fail(TRUSS_EINVAL, me + ": NULL argument");
  for (int i = 0; i < n_fields; ++i) {
    const truss_replay_field_t &f = fields[i];
    if (!f.ring || !f.ext) return tb_fail(TRUSS_EINVAL, me + ": a field's ring / ext pointer is NULL");
    if (((size_t)f.ring | (size_t)f.ext) & 3) return tb_fail(TRUSS_EINVAL, me + ": float pointers must be 4-byte aligned");
    if (f.ext_row_stride < 0 || f.ext_part_stride < 0 || f.ext_rows < 0) return tb_fail(TRUSS_EINVAL, me + ": negative stride / row count");
    if (gather ? f.ext_rows < k : (f.group < 0 || f.group > 3)) return tb_fail(TRUSS_EINVAL, me + (gather ? ": an output has fewer rows than the batch" : ": group outside 0..3"));
    long per_row;
    if (f.nbr) {
      if (f.k_nbr > 16) return tb_fail(TRUSS_EUNSUPPORTED, me + ": k_nbr <= 16");
      if (f.n < 1 || f.n > 32767 || f.k_nbr < 1) return tb_fail(TRUSS_EINVAL, me + ": pattern field needs n 1..32767, k_nbr 1..16");
      per_row = gather ? ((long)f.n * f.n + 3) / 4 : ((long)f.n * f.k_nbr + 3) / 4;
    } else {
      if (f.parts < 1 || f.part_len < 1 || (long)f.parts * f.part_len > 0x7fffffffL) return tb_fail(TRUSS_EINVAL, me + ": plain field needs parts, part_len >= 1");
      per_row = (long)f.parts * ((f.part_len + 3L) / 4);
    }
    if (per_row * k >= (1L << 31)) return tb_fail(TRUSS_EUNSUPPORTED, me + ": rows x row pieces of one field must stay below 2^31");
  }
  hipStream_t st = (hipStream_t)stream;
  for (int i0 = 0; i0 < n_fields; i0 += TRP_MAX) {
    const int nf = n_fields - i0 < TRP_MAX ? n_fields - i0 : TRP_MAX;
    ReplayDev D;
    memset(&D, 0, sizeof D);
    D.rows = (const long long *)rows;
    D.head = head;
    D.capacity = capacity;
    D.k = k;
    unsigned gx = 1;
    for (int i = 0; i < nf; ++i) {
      const truss_replay_field_t &f = fields[i0 + i];
      ReplayFieldDev &P = D.f[i];
      P.ring = (uint32_t *)f.ring;
      P.ext = (uint32_t *)f.ext;
      P.nbr = f.nbr;
      P.ext_rows = f.ext_rows;
      P.ext_row_stride = f.ext_row_stride;
      P.group = f.group;
      if (f.nbr) {
        P.n = f.n;
        P.k_nbr = f.k_nbr;
        P.ring_row = f.n * f.k_nbr;
        P.pp = 1;
        P.per_row = (unsigned)(gather ? ((long)f.n * f.n + 3) / 4 : ((long)f.n * f.k_nbr + 3) / 4);
      } else {
        P.part_len = f.part_len;
        P.ext_part_stride = f.parts > 1 ? f.ext_part_stride : 0;
        P.ring_row = f.parts * f.part_len;
        P.pp = (unsigned)((f.part_len + 3) / 4);
        P.per_row = (unsigned)f.parts * P.pp;
      }
      const long blocks = ((long)P.per_row * k + 255) / 256;
      P.nblocks = (unsigned)(blocks < TRP_BLOCKS ? blocks : TRP_BLOCKS);
      gx = P.nblocks > gx ? P.nblocks : gx;
    }
    if (gather)
      hipLaunchKernelGGL(truss_replay_kernel<true>, dim3(gx, (unsigned)nf), dim3(256), 0, st, D);
    else
      hipLaunchKernelGGL(truss_replay_kernel<false>, dim3(gx, (unsigned)nf), dim3(256), 0, st, D);
    if (int rc = tb_launched((me + " kernel launch failed: ").c_str())) return rc;
  }
  return TRUSS_OK;
}

extern "C" int truss_replay_scatter(const truss_replay_field_t *fields, int32_t n_fields, const int64_t *rows, int32_t k, int64_t head,
                                    int64_t capacity, void *stream) {
  return trp_run("truss_replay_scatter", false, fields, n_fields, rows, k, head, capacity, stream);
}

extern "C" int truss_replay_gather(const truss_replay_field_t *fields, int32_t n_fields, const int64_t *idx, int32_t batch, int64_t capacity,
                                   void *stream) {
  return trp_run("truss_replay_gather", true, fields, n_fields, idx, batch, 0, capacity, stream);
}
