// truss_archive.h -- the archive update of a game step as one launch (include/truss_mi355.h, truss_archive_merge).
// On top the host-side argument check; below it, for the device compiler only, the gfx950 kernel (truss_archive_kernel<64> / <256>)
// and the C entry.  truss_hip.hip includes this file after truss_reward.h.
// The cull, ordering, crowding truncation, metrics and closed-form hypervolume are those of truss_front_kernel (truss_front.h is the
// source of the algorithm); this header carries its own copy of that device code on purpose.
#pragma once
#include <cstdint>
#include <string>

static int tb_fail(int code, const std::string &msg);

static inline int tb_archive_check(const truss_archive_args_t *a) {
  if (!a || a->struct_size != sizeof(truss_archive_args_t)) return tb_fail(TRUSS_EINVAL, "truss_archive_merge: bad args / struct_size");
  if (a->n_envs < 0) return tb_fail(TRUSS_EINVAL, "truss_archive_merge: n_envs < 0");
  if (a->max_points < 1 || a->n_slots < 0 || (int64_t)a->max_points + a->n_slots > TRUSS_ARCHIVE_MAXROWS)
    return tb_fail(TRUSS_EINVAL, "truss_archive_merge: max_points >= 1, n_slots >= 0 and max_points + n_slots <= 256 rows per env");
  if (a->max_front == 1 || a->max_front < 0) return tb_fail(TRUSS_EINVAL, "truss_archive_merge: max_front must be 0 (no truncation) or >= 2");
  const int32_t P = a->max_points, C = a->n_slots;
  if (a->max_out < (a->max_front ? a->max_front : P + C))
    return tb_fail(TRUSS_EINVAL, "truss_archive_merge: max_out is smaller than the front can get (max_front when truncating, max_points + n_slots otherwise)");
  if (a->n_y < 1 || a->n_sec < 1) return tb_fail(TRUSS_EINVAL, "truss_archive_merge: n_y / n_sec < 1");
  const int64_t widest = a->n_y > a->n_sec ? a->n_y : a->n_sec;
  if ((int64_t)a->max_out * ((widest + 3) / 4) > INT32_MAX) return tb_fail(TRUSS_EINVAL, "truss_archive_merge: max_out x row pieces >= 2^31");
  if (a->n_cand_rows < 0) return tb_fail(TRUSS_EINVAL, "truss_archive_merge: n_cand_rows < 0");
  const size_t B = (size_t)a->n_envs;
  if (!a->slot_row && (int64_t)a->n_cand_rows < (int64_t)a->n_envs * C)
    return tb_fail(TRUSS_EINVAL, "truss_archive_merge: slot_row NULL needs n_cand_rows >= n_envs x n_slots candidate rows");
  if (B == 0) return TRUSS_OK;
  if (!a->pts_in || !a->n_in || !a->y_in || !a->sec_in) return tb_fail(TRUSS_EINVAL, "truss_archive_merge: pts_in / n_in / y_in / sec_in NULL");
  if (C > 0 && (!a->cand_points || !a->cand_y || !a->cand_sec)) return tb_fail(TRUSS_EINVAL, "truss_archive_merge: cand_points / cand_y / cand_sec NULL");
  if (!a->pts_out || !a->y_out || !a->sec_out || !a->n_out) return tb_fail(TRUSS_EINVAL, "truss_archive_merge: pts_out / y_out / sec_out / n_out NULL");
  // outputs must not overlap the inputs or each other: a workgroup reads its env's rows while it writes them, in another order
  struct Range { const void *p; size_t bytes; const char *name; };
  const size_t R = C > 0 ? (size_t)a->n_cand_rows : 0, O = (size_t)a->max_out, ny = (size_t)a->n_y, ns = (size_t)a->n_sec;
  const Range in[] = {{a->pts_in, B * P * 32, "pts_in"}, {a->n_in, B * 4, "n_in"}, {a->y_in, B * P * ny * 4, "y_in"}, {a->sec_in, B * P * ns * 4, "sec_in"},
                      {a->slot_row, B * C * 4, "slot_row"}, {a->cand_points, R * 32, "cand_points"}, {a->cand_y, R * ny * 4, "cand_y"},
                      {a->cand_sec, R * ns * 4, "cand_sec"}};
  const Range out[] = {{a->pts_out, B * O * 32, "pts_out"}, {a->y_out, B * O * ny * 4, "y_out"}, {a->sec_out, B * O * ns * 4, "sec_out"},
                       {a->n_out, B * 4, "n_out"}, {a->accepted, B * C, "accepted"}, {a->front_idx, B * O * 4, "front_idx"},
                       {a->hv_front, B * 8, "hv_front"}, {a->metrics, B * 40, "metrics"}};
  auto overlap = [](const Range &u, const Range &v) {
    if (!u.p || !v.p || !u.bytes || !v.bytes) return false;
    const uintptr_t u0 = (uintptr_t)u.p, v0 = (uintptr_t)v.p;
    return u0 < v0 + v.bytes && v0 < u0 + u.bytes;
  };
  const int n_in = (int)(sizeof in / sizeof in[0]), n_out = (int)(sizeof out / sizeof out[0]);
  for (int o = 0; o < n_out; ++o) {
    for (int k = 0; k < n_in; ++k)
      if (overlap(out[o], in[k])) return tb_fail(TRUSS_EINVAL, std::string("truss_archive_merge: output ") + out[o].name + " overlaps input " + in[k].name);
    for (int k = 0; k < o; ++k)
      if (overlap(out[o], out[k])) return tb_fail(TRUSS_EINVAL, std::string("truss_archive_merge: output ") + out[o].name + " overlaps output " + out[k].name);
  }
  return TRUSS_OK;
}

#ifdef __HIPCC__
// Rows of `width` 32-bit words, copied by the whole workgroup: output row j < nf comes from the archive (input row keep[j] < P) or from
// the candidate arrays (row crow[keep[j]]), every other row is zeros.  The unit of work is a piece of four words: one 16-byte load
// and store where the piece is whole and both addresses allow it, word by word otherwise (the tail of a row, odd widths, odd bases).
template <int NT>
__device__ __forceinline__ void tb_ar_copy_rows(uint32_t *dst, const uint32_t *arch, const uint32_t *cand, int width, int max_out, int nf,
                                                int P, const int *keep, const int *crow, int tid) {
  const int npc = (width + 3) >> 2, total = max_out * npc;
  for (int t = tid; t < total; t += NT) {
    const int j = t / npc, w0 = 4 * (t - j * npc);
    const int nw = width - w0 < 4 ? width - w0 : 4;
    uint32_t *d = dst + (size_t)j * width + w0;
    const bool dvec = nw == 4 && ((uintptr_t)d & 15) == 0;
    if (j < nf) {
      const int kid = keep[j];
      const uint32_t *s = (kid < P ? arch + (size_t)kid * width : cand + (size_t)crow[kid] * width) + w0;
      if (dvec && ((uintptr_t)s & 15) == 0) {
        *(uint4 *)d = *(const uint4 *)s;
      } else {
        for (int q = 0; q < nw; ++q) d[q] = s[q];
      }
    } else if (dvec) {
      *(uint4 *)d = make_uint4(0u, 0u, 0u, 0u);
    } else {
      for (int q = 0; q < nw; ++q) d[q] = 0u;
    }
  }
}

// One workgroup of NT threads per env, thread i <-> row i of the cull (P archive rows, then C candidate slots; P + C <= NT): NT = 64,
// one wave, for the train game's chunks, NT = 256 for the design game's step-wide cull.  The selection is truss_front_kernel<NT>'s,
// statement for statement (quadratic parts as loops over LDS broadcast reads; ballot / popcount -- with NT > 64 plus a prefix over the
// waves' popcounts through LDS -- for the front's size and the compaction after truncation; the order-sensitive float64 sums by
// thread 0 in index order).  What is new is around it: the rows are gathered from the archive and, through slot_row, from the
// candidate arrays as they lie; the surviving rows, designs and flags are written by the threads that own them.  All barriers are
// at the top level of the kernel: all NT threads reach every one of them.
template <int NT>
__global__ __launch_bounds__(NT) void truss_archive_kernel(const truss_archive_args_t A) {
  __shared__ double px[NT], py[NT], pc1[NT], pc2[NT];      // the rows the cull sees
  __shared__ double sx[NT], sy[NT], sd[NT], scr[NT];        // front sorted by obj1; distances; crowding
  __shared__ int sidx[NT], keep[NT];
  __shared__ int crow[NT], infront[NT];                     // candidate-array row of input row i (-1: none); 1 if row i is in the new archive
  __shared__ int wcnt[2][NT / 64];                          // per-wave popcounts: front rows, kept rows (used with NT > 64 only)
  const int b = blockIdx.x, i = threadIdx.x, P = A.max_points, C = A.n_slots, n = P + C;
  const int wave = i >> 6, lane = i & 63;
  int na = A.n_in[b];
  na = na < 0 ? 0 : (na > P ? P : na);
  const bool have = i < n;
  double x = 0.0, y = 0.0, c1 = 2.0, c2 = 0.0;              // an empty slot is the infeasible row [0, 0, 2, 0]
  int cr = -1;
  if (i < P) {
    const double *row = A.pts_in + ((size_t)b * P + i) * 4;
    x = row[0]; y = row[1]; c1 = row[2]; c2 = row[3];
    if (i >= na) c1 = 2.0;                                   // dead archive row: infeasible marker
  } else if (have) {
    const int c = i - P;
    const int r = A.slot_row ? A.slot_row[(size_t)b * C + c] : b * C + c;
    if (r >= 0 && r < A.n_cand_rows) {
      const double *row = A.cand_points + (size_t)r * 4;
      x = row[0]; y = row[1]; c1 = row[2]; c2 = row[3];
      if (!(c1 <= 1.0 && c2 <= 1.0)) c1 = 2.0;               // not ok (a NaN is not ok): its own values, marked infeasible
      cr = r;
    }
  }
  px[i] = x; py[i] = y; pc1[i] = c1; pc2[i] = c2;
  crow[i] = cr; infront[i] = 0;
  __syncthreads();
  const bool feas = have && !(c1 > 1.0 || c2 > 1.0);
  bool dom = false, dup = false;
  for (int j = 0; j < n; ++j) {
    const bool fj = !(pc1[j] > 1.0 || pc2[j] > 1.0);
    dom |= fj && px[j] < x && py[j] < y;
    dup |= fj && j < i && px[j] == x && py[j] == y && pc1[j] == c1 && pc2[j] == c2;
  }
  const bool fr = feas && !dom && !dup;
  keep[i] = fr ? 1 : 0;
  if constexpr (NT > 64) {
    const int wf = __popcll(__ballot(fr));
    if (lane == 0) wcnt[0][wave] = wf;
  }
  __syncthreads();
  // position in the front sorted by (obj1, obj2, input order)
  int rank = 0;
  for (int j = 0; j < n; ++j) rank += keep[j] && (px[j] < x || (px[j] == x && (py[j] < y || (py[j] == y && j < i))));
  int nf = 0;                                               // size of the front: the waves' popcounts, or the one wave's own
  if constexpr (NT > 64) {
    for (int w = 0; w < NT / 64; ++w) nf += wcnt[0][w];
  }
  __syncthreads();
  if constexpr (NT == 64) nf = __popcll(__ballot(fr));
  if (fr) { sx[rank] = x; sy[rank] = y; sidx[rank] = i; }
  __syncthreads();
  // crowding distance on the sorted front (utils.py:96-110)
  if (i + 1 < nf) {
    const double dx = sx[i] - sx[i + 1], dy = sy[i] - sy[i + 1];
    sd[i] = sqrt(dx * dx + dy * dy);
  }
  __syncthreads();
  if (i < nf) scr[i] = nf == 1 ? 0.0 : (i == 0 ? sd[0] : (i == nf - 1 ? sd[nf - 2] : sd[i - 1] + sd[i]));
  __syncthreads();
  // truncation to max_front: both ends + the interior points of largest crowding distance (ties: position)
  bool kp = i < nf;
  if (A.max_front != 0 && nf > A.max_front) {
    if (i > 0 && i < nf - 1) {
      int cr2 = 0;
      for (int j = 1; j < nf - 1; ++j) cr2 += (scr[j] > scr[i] || (scr[j] == scr[i] && j < i));
      kp = cr2 < A.max_front - 2;
    }
  }
  const unsigned long long kmask = __ballot(kp);
  if constexpr (NT > 64) {
    if (lane == 0) wcnt[1][wave] = __popcll(kmask);
  }
  const double kx = i < nf ? sx[i] : 0.0, ky = i < nf ? sy[i] : 0.0;
  const int kid = i < nf ? sidx[i] : -1;
  __syncthreads();
  int pos = __popcll(kmask & ((1ull << lane) - 1ull)), nk = __popcll(kmask);
  if constexpr (NT > 64) {
    nk = 0;
    for (int w = 0; w < NT / 64; ++w) {
      pos += w < wave ? wcnt[1][w] : 0;
      nk += wcnt[1][w];
    }
  }
  if (kp) { sx[pos] = kx; sy[pos] = ky; keep[pos] = kid; infront[kid] = 1; }   // kid: one front row per thread, kp implies i < nf
  nf = nk;
  __syncthreads();
  if (i + 1 < nf) {
    const double dx = sx[i] - sx[i + 1], dy = sy[i] - sy[i + 1];
    sd[i] = sqrt(dx * dx + dy * dy);
  }
  // ---- the new archive: rows in front order, zeros behind them; every element written by one thread ----
  const int O = A.max_out;
  for (int j = i; j < O; j += NT) {
    double o0 = 0.0, o1 = 0.0, o2 = 0.0, o3 = 0.0;
    int src = -1;
    if (j < nf) {
      src = keep[j];
      o0 = px[src]; o1 = py[src]; o2 = pc1[src]; o3 = pc2[src];
      o0 = o0 > 1.0 ? 1.0 : o0;                              // :434-436 (torch.clamp(max=1): a NaN goes through)
      o1 = o1 > 1.0 ? 1.0 : o1;
    }
    double *q = A.pts_out + ((size_t)b * O + j) * 4;
    q[0] = o0; q[1] = o1; q[2] = o2; q[3] = o3;
    if (A.front_idx) A.front_idx[(size_t)b * O + j] = src;
  }
  if (A.accepted && i >= P && have) A.accepted[(size_t)b * C + (i - P)] = (uint8_t)infront[i];
  if (i == 0) A.n_out[b] = nf;
  __syncthreads();
  if (i == 0 && (A.metrics || A.hv_front)) {
    if (A.metrics) {
      double maxd = 0.0, disd = 1.0, sumd = 0.0, stdcd = 1.0, pn = 0.0;
      if (nf >= 2) {
        maxd = sd[0];
        for (int k = 0; k < nf - 1; ++k) { maxd = sd[k] > maxd ? sd[k] : maxd; sumd += sd[k]; }
        double acc = 0.0;
        const double ctr = maxd / (nf - 1);            // sic: the reference centres on max/len (utils.py:131)
        for (int k = 0; k < nf - 1; ++k) acc += (sd[k] - ctr) * (sd[k] - ctr);
        disd = sqrt(acc / (nf - 1));
      }
      if (nf > 3) {
        double s = 0.0, mx = 0.0;
        for (int k = 1; k < nf - 1; ++k) {
          const double cd = fabs(sx[k - 1] - sx[k + 1]) + fabs(sy[k - 1] - sy[k + 1]);
          scr[k] = cd; s += cd; mx = cd > mx ? cd : mx;
        }
        if (s != 0.0) {
          const int m = nf - 2;
          double mean = 0.0;
          for (int k = 1; k < nf - 1; ++k) { scr[k] = scr[k] / mx; mean += scr[k]; }
          mean /= m;
          double var = 0.0, p10 = 0.0;
          for (int k = 1; k < nf - 1; ++k) {
            const double v = scr[k], d = v - mean;
            var += d * d;
            const double v2 = v * v, v4 = v2 * v2;
            p10 += v4 * v4 * v2;
          }
          stdcd = sqrt(var / m);
          pn = pow(p10, 0.1);
        }
      }
      double *M = A.metrics + (size_t)b * 5;
      M[0] = maxd; M[1] = disd; M[2] = pn; M[3] = sumd; M[4] = stdcd;
    }
    if (A.hv_front) {      // the front is sorted by obj1 and its obj2 decreases: closed form of the union area, reference point (1, 1)
      const double rx = 1.0, ry = 1.0;
      double hv = 0.0;
      if (nf > 0 && !(nf == 1 && sx[0] == 1.0 && sy[0] == 1.0)) {
        double area = 0.0, runmin = 1.0, minx = sx[0], miny = sy[0];
        for (int k = 0; k < nf; ++k) {
          const double cxk = fmin(sx[k], 1.0), cyk = fmin(sy[k], 1.0);
          runmin = cyk < runmin ? cyk : runmin;
          const double nx = k + 1 < nf ? fmin(sx[k + 1], 1.0) : 1.0;
          area += (nx - cxk) * (1.0 - runmin);
          minx = sx[k] < minx ? sx[k] : minx;
          miny = sy[k] < miny ? sy[k] : miny;
        }
        hv = area - ((1.0 - rx) * (1.0 - minx) + (1.0 - ry) * (1.0 - miny) - (1.0 - rx) * (1.0 - ry));
      }
      A.hv_front[b] = hv;
    }
  }
  // the surviving designs (the other waves copy while thread 0 sums: the copy reads keep[] / crow[] only)
  tb_ar_copy_rows<NT>((uint32_t *)A.y_out + (size_t)b * O * A.n_y, (const uint32_t *)A.y_in + (size_t)b * P * A.n_y, (const uint32_t *)A.cand_y,
                      A.n_y, O, nf, P, keep, crow, i);
  tb_ar_copy_rows<NT>((uint32_t *)A.sec_out + (size_t)b * O * A.n_sec, (const uint32_t *)A.sec_in + (size_t)b * P * A.n_sec,
                      (const uint32_t *)A.cand_sec, A.n_sec, O, nf, P, keep, crow, i);
}

extern "C" int truss_archive_merge(const truss_archive_args_t *a, void *stream) {
  if (int rc = tb_archive_check(a)) return rc;
  if (a->n_envs == 0) return TRUSS_OK;
  if (a->max_points + a->n_slots <= 64)
    hipLaunchKernelGGL(truss_archive_kernel<64>, dim3((unsigned)a->n_envs), dim3(64), 0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(truss_archive_kernel<256>, dim3((unsigned)a->n_envs), dim3(256), 0, (hipStream_t)stream, *a);
  return tb_launched("archive kernel launch failed: ");
}
#endif  // __HIPCC__
