// truss_reward.h -- the difference reward of a game step as one launch (include/truss_mi355.h, truss_reward).
// On top the host-side argument check; below it, for the device compiler only, the gfx950 kernel (truss_reward_kernel) and the
// C entry.  truss_hip.hip includes this file after truss_front.h.
// The cull, ordering, crowding truncation and closed-form hypervolume are those of truss_front_kernel<64> (truss_front.h is the
// source of the algorithm); this header carries its own copy of that device code on purpose.
#pragma once
#include <cstdint>
#include <string>

static int tb_fail(int code, const std::string &msg);

static inline int tb_reward_check(const truss_reward_args_t *a) {
  if (!a || a->struct_size != sizeof(truss_reward_args_t)) return tb_fail(TRUSS_EINVAL, "truss_reward: bad args / struct_size");
  if (a->n_sets < 0) return tb_fail(TRUSS_EINVAL, "truss_reward: n_sets < 0");
  if (a->max_points < 1 || a->max_points + 3 > 64) return tb_fail(TRUSS_EINVAL, "truss_reward: max_points must be 1..61 (max_points + 3 rows per wave)");
  if (a->max_front == 1 || a->max_front < 0) return tb_fail(TRUSS_EINVAL, "truss_reward: max_front must be 0 (no truncation) or >= 2");
  if (!a->front_no || !a->n_front_no || !a->pf_hv || !a->n_pf_hv || !a->parent || !a->points || !a->ref_points || !a->n_pf)
    return tb_fail(TRUSS_EINVAL, "truss_reward: an input pointer is NULL");
  if (!a->R || !a->G_U || !a->xmax || !a->ymax) return tb_fail(TRUSS_EINVAL, "truss_reward: R / G_U / xmax / ymax NULL");
  return TRUSS_OK;
}

#ifdef __HIPCC__
// torch.clamp(v, min=lo) / torch.maximum: a NaN goes through
__device__ __forceinline__ double tb_rw_clamp_min(double v, double lo) { return v < lo ? lo : v; }
__device__ __forceinline__ double tb_rw_clamp_max(double v, double hi) { return v > hi ? hi : v; }
__device__ __forceinline__ double tb_rw_maximum(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

// One workgroup of 256 threads per (env, member) pair k.  Wave s (0..2) owns the point set "archive + the feasible new points of
// the agents other than s", wave 3 the set with all three; lane i owns row i of its wave's set (at most P + 3 <= 64 rows).  The
// archive rows, the pf_hv rows and the three points are read from HBM once, by the whole workgroup, into LDS; every wave then runs
// the one-wave form of the front kernel on LDS arrays of its own ([wave][row]): ballot / popcount give the front's size and the
// compaction after truncation, everything quadratic is a loop over LDS broadcast reads, and the order-sensitive float64 sums
// (distances, crowding mean / variance, union area) are accumulated by the wave's lane 0 in index order, like the front kernel's
// thread 0.  Wave 0 also sorts the pf_hv rows by clipped x for the two hv_all values.  Nothing crosses waves before the last
// barrier; all barriers are at the top level of the kernel, so all 256 threads reach every one of them.  Thread 0 then evaluates
// the reward expressions of reward.py (difference_reward, the lines after the three launches) in their order of operations.
__global__ __launch_bounds__(256) void truss_reward_kernel(const truss_reward_args_t A) {
  __shared__ double arow[256], hrow[256], spt[12];           // archive rows, pf_hv rows ([row][4]); the three points
  __shared__ double s_px[4][64], s_py[4][64], s_pc1[4][64], s_pc2[4][64];   // the wave's point set
  __shared__ double s_sx[4][64], s_sy[4][64], s_sd[4][64], s_scr[4][64];    // its front sorted by obj1; distances; crowding
  __shared__ int s_keep[4][64];
  __shared__ double ax[64], ay[64];                           // pf_hv rows sorted by clipped x
  __shared__ double res[8];                                   // the parts: hv of the four sets, compareV, real_compareV, sum_distance, std_cd
  const int k = blockIdx.x, t = threadIdx.x, P = A.max_points;
  const int wave = t >> 6, i = t & 63;
  double *px = s_px[wave], *py = s_py[wave], *pc1 = s_pc1[wave], *pc2 = s_pc2[wave];
  double *sx = s_sx[wave], *sy = s_sy[wave], *sd = s_sd[wave], *scr = s_scr[wave];
  int *keep = s_keep[wave];
  if (t < 4 * P) {                                            // 4 P <= 244 < 256
    arow[t] = A.front_no[(size_t)k * P * 4 + t];
    hrow[t] = A.pf_hv[(size_t)k * P * 4 + t];
  }
  if (t < 12) spt[t] = A.points[(size_t)k * 12 + t];
  int n0 = A.n_front_no[k], m = A.n_pf_hv[k];
  n0 = n0 < 0 ? 0 : (n0 > P ? P : n0);
  m = m < 0 ? 0 : (m > P ? P : m);
  __syncthreads();
  // _feasible: all four entries <= 1 (a NaN is infeasible)
  const bool f0 = spt[0] <= 1.0 && spt[1] <= 1.0 && spt[2] <= 1.0 && spt[3] <= 1.0;
  const bool f1 = spt[4] <= 1.0 && spt[5] <= 1.0 && spt[6] <= 1.0 && spt[7] <= 1.0;
  const bool f2 = spt[8] <= 1.0 && spt[9] <= 1.0 && spt[10] <= 1.0 && spt[11] <= 1.0;
  // the wave's set: the archive rows, then the feasible points of the agents it does not leave out, in agent order
  const bool u0 = f0 && wave != 0, u1 = f1 && wave != 1, u2 = f2 && wave != 2;
  const int n = n0 + (u0 ? 1 : 0) + (u1 ? 1 : 0) + (u2 ? 1 : 0);
  const bool have = i < n;
  const int e = i - n0;                                       // which of the appended points (have && e >= 0)
  const int ag = e <= 0 ? (u0 ? 0 : (u1 ? 1 : 2)) : (e == 1 ? (u0 && u1 ? 1 : 2) : 2);
  const double *row = i < n0 ? arow + 4 * i : spt + 4 * ag;
  const double x = have ? row[0] : 0.0, y = have ? row[1] : 0.0, c1 = have ? row[2] : 0.0, c2 = have ? row[3] : 0.0;
  px[i] = x; py[i] = y; pc1[i] = c1; pc2[i] = c2;
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
  __syncthreads();
  // position in the front sorted by (obj1, obj2, input order)
  int rank = 0;
  for (int j = 0; j < n; ++j) rank += keep[j] && (px[j] < x || (px[j] == x && (py[j] < y || (py[j] == y && j < i))));
  int nf = __popcll(__ballot(fr));
  if (fr) { sx[rank] = x; sy[rank] = y; }
  // wave 0: the pf_hv rows by clipped x (ties: input order)
  const bool hhave = wave == 0 && i < m;
  if (hhave) {
    const double hx = fmin(hrow[4 * i], 1.0), hy = fmin(hrow[4 * i + 1], 1.0);
    int arank = 0;
    for (int j = 0; j < m; ++j) {
      const double hxj = fmin(hrow[4 * j], 1.0);
      arank += (hxj < hx || (hxj == hx && j < i));
    }
    ax[arank] = hx; ay[arank] = hy;
  }
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
      int cr = 0;
      for (int j = 1; j < nf - 1; ++j) cr += (scr[j] > scr[i] || (scr[j] == scr[i] && j < i));
      kp = cr < A.max_front - 2;
    }
  }
  const unsigned long long kmask = __ballot(kp);
  const double kx = i < nf ? sx[i] : 0.0, ky = i < nf ? sy[i] : 0.0;
  __syncthreads();
  const int pos = __popcll(kmask & ((1ull << i) - 1ull));
  if (kp) { sx[pos] = kx; sy[pos] = ky; }
  nf = __popcll(kmask);
  __syncthreads();
  if (i + 1 < nf) {
    const double dx = sx[i] - sx[i + 1], dy = sy[i] - sy[i + 1];
    sd[i] = sqrt(dx * dx + dy * dy);
  }
  __syncthreads();
  const double rx = A.ref_points[2 * (size_t)k], ry = A.ref_points[2 * (size_t)k + 1];
  if (i == 0) {
    if (wave == 3) {            // sum_distance and std_cd of the full set (utils.py:126-214)
      double sumd = 0.0, stdcd = 1.0;
      if (nf >= 2) {
        for (int q = 0; q < nf - 1; ++q) sumd += sd[q];
      }
      if (nf > 3) {
        double s = 0.0, mx = 0.0;
        for (int q = 1; q < nf - 1; ++q) {
          const double cd = fabs(sx[q - 1] - sx[q + 1]) + fabs(sy[q - 1] - sy[q + 1]);
          scr[q] = cd; s += cd; mx = cd > mx ? cd : mx;
        }
        if (s != 0.0) {
          const int mm = nf - 2;
          double mean = 0.0;
          for (int q = 1; q < nf - 1; ++q) { scr[q] = scr[q] / mx; mean += scr[q]; }
          mean /= mm;
          double var = 0.0;
          for (int q = 1; q < nf - 1; ++q) {
            const double d = scr[q] - mean;
            var += d * d;
          }
          stdcd = sqrt(var / mm);
        }
      }
      res[6] = sumd; res[7] = stdcd;
    }
    {                           // the front is sorted by obj1 and its obj2 decreases: closed form of the union area
      double hv = 0.0;
      if (nf > 0 && !(nf == 1 && sx[0] == 1.0 && sy[0] == 1.0)) {
        double area = 0.0, runmin = 1.0, minx = sx[0], miny = sy[0];
        for (int q = 0; q < nf; ++q) {
          const double cxq = fmin(sx[q], 1.0), cyq = fmin(sy[q], 1.0);
          runmin = cyq < runmin ? cyq : runmin;
          const double nx = q + 1 < nf ? fmin(sx[q + 1], 1.0) : 1.0;
          area += (nx - cxq) * (1.0 - runmin);
          minx = sx[q] < minx ? sx[q] : minx;
          miny = sy[q] < miny ? sy[q] : miny;
        }
        hv = area - ((1.0 - rx) * (1.0 - minx) + (1.0 - ry) * (1.0 - miny) - (1.0 - rx) * (1.0 - ry));
      }
      res[wave] = hv;
    }
    if (wave == 0) {            // hv_all of the pf_hv rows: with the reference point (compareV) and with (1, 1) (real_compareV)
      double cv = 0.0, rcv = 0.0;
      if (m > 0 && !(m == 1 && hrow[0] == 1.0 && hrow[1] == 1.0)) {
        double area = 0.0, runmin = 1.0, minx = hrow[0], miny = hrow[1];
        for (int q = 0; q < m; ++q) {
          runmin = ay[q] < runmin ? ay[q] : runmin;
          const double nx = q + 1 < m ? ax[q + 1] : 1.0;
          area += (nx - ax[q]) * (1.0 - runmin);
          minx = hrow[4 * q] < minx ? hrow[4 * q] : minx;
          miny = hrow[4 * q + 1] < miny ? hrow[4 * q + 1] : miny;
        }
        cv = area - ((1.0 - rx) * (1.0 - minx) + (1.0 - ry) * (1.0 - miny) - (1.0 - rx) * (1.0 - ry));
        rcv = area - ((1.0 - 1.0) * (1.0 - minx) + (1.0 - 1.0) * (1.0 - miny) - (1.0 - 1.0) * (1.0 - 1.0));
      }
      res[4] = cv; res[5] = rcv;
    }
  }
  __syncthreads();
  if (t != 0) return;
  const double compareV = res[4], real_compareV = res[5], sum_distance = res[6], std_cd = res[7];
  if (A.parts) {
    double *Q = A.parts + (size_t)k * 8;
    for (int q = 0; q < 8; ++q) Q[q] = res[q];
  }
  const double hyperV = tb_rw_clamp_min(res[3] - compareV, 0.0);
  const double npf = (double)A.n_pf[k];
  const double mcl = tb_rw_clamp_min(real_compareV, 0.25);
  const double par0 = A.parent[2 * (size_t)k], par1 = A.parent[2 * (size_t)k + 1];
  const double mn = mcl * npf;
  const double t3 = 10.0 * (real_compareV / npf);
  const double t4 = 0.05 * tb_rw_clamp_max(tb_rw_clamp_min(std_cd, 0.0), 1.0) / npf;
  const double t5 = 0.05 * sum_distance / (2.0 * sqrt(mcl) * npf);
  const double ninf = -__builtin_huge_val();
  double xm = ninf, ym = ninf;
  for (int j = 0; j < 3; ++j) {
    const bool fj = j == 0 ? f0 : (j == 1 ? f1 : f2);
    const double c0 = j == 0 ? 1.0 : (j == 1 ? 0.5 : 0.0);    // coef[j][0]; coef[j][1] = 1 - coef[j][0]
    const double p0 = spt[4 * j], p1 = spt[4 * j + 1];
    const double hvj = tb_rw_clamp_min(res[j] - compareV, 0.0);
    double w = c0 * tb_rw_clamp_min(par0 - p0, 0.0) + (1.0 - c0) * tb_rw_clamp_min(par1 - p0, 0.0);   // both terms use point[0] (master...:348-352)
    w = fj ? w : 0.0;
    A.R[(size_t)k * 3 + j] = 0.25 * w / mn + 0.25 * (hyperV - hvj) / mn + t3 - t4 + t5;
    xm = tb_rw_maximum(xm, fj ? p0 : ninf);
    ym = tb_rw_maximum(ym, fj ? p1 : ninf);
  }
  A.G_U[k] = 20.0 * real_compareV / npf - std_cd / npf + sum_distance / npf;
  A.xmax[k] = tb_rw_maximum(par0, xm);
  A.ymax[k] = tb_rw_maximum(par1, ym);
}

extern "C" int truss_reward(const truss_reward_args_t *a, void *stream) {
  if (int rc = tb_reward_check(a)) return rc;
  if (a->n_sets == 0) return TRUSS_OK;
  hipLaunchKernelGGL(truss_reward_kernel, dim3((unsigned)a->n_sets), dim3(256), 0, (hipStream_t)stream, *a);
  return tb_launched("reward kernel launch failed: ");
}
#endif  // __HIPCC__
