// The steps that objective.hip (the cell search and the value kernel) and
// objective_grad.hip (value and gradient by the adjoint method) have in common, each
// stated once: the arm's tables, the cell record's layout, the rotational taps, the
// template guard, the spline chunks' hand-over, a pixel's knot interval and spline
// piece, the value/status tail, the wave reduction of the normal-equation sums.
#pragma once
#include "template_dev.h"
#include "objective_sum.h"

#define TRI(i, j) ((i) * ((i) + 1) / 2 + (j))

// (tools/perf/obj_bench.hip builds one npoly only: -DOBJ_ONLY_P=10)
#ifdef OBJ_ONLY_P
#define RVS_ALL_CASES RVS_CASE(OBJ_ONLY_P)
#else
#define RVS_ALL_CASES                                                     \
  RVS_CASE(1) RVS_CASE(2) RVS_CASE(3) RVS_CASE(4) RVS_CASE(5) RVS_CASE(6) \
  RVS_CASE(7) RVS_CASE(8) RVS_CASE(9) RVS_CASE(10) RVS_CASE(11)           \
  RVS_CASE(12) RVS_CASE(13) RVS_CASE(14) RVS_CASE(15) RVS_CASE(16)
#endif

// the grid of spectrum s on an arm (rvs_point_arm.grid_id, include/rvsgpu.h):
// wavelengths, pixel knot coordinates, basis, base of the per-spectrum blocks of
// the rvs_chisq_prepare buffer
struct ObjArmGrid {
  const double *lam, *pix, *polysT, *wbase;
  const double2 *lp;   // {lam, pix} of the grid's pixels (rvs_chisq_prepare)
  // {1/e, s/e} of spectrum s's pixels (rvs_chisq_prepare's second table: e with the
  // systematic floor of `espec_sys` in quadrature, 0 / 0 on the padding of a short
  // grid): one 16-byte load where every evaluation used to take a square root, a
  // division and a product per pixel -- the same operations, done once per batch
  const double2 *sig;
};
__device__ __forceinline__ ObjArmGrid obj_arm_grid(const rvs_point_arm &T, int s) {
  ObjArmGrid g;
  const int G = T.G > 1 ? T.G : 1;
  const int64_t gi = (T.G > 1 && T.grid_id) ? T.grid_id[s] : 0;
  g.lam = T.lam + gi * T.npix;
  g.pix = T.work + gi * T.npix;
  g.polysT = T.polysT + gi * T.polys_stride;
  g.wbase = T.work + (int64_t)G * T.npix;
  g.lp = reinterpret_cast<const double2 *>(g.wbase + 4ll * T.S * T.npix + 2ll * T.S) +
         gi * T.npix;
  g.sig = reinterpret_cast<const double2 *>(g.wbase + 2ll * T.S * T.npix + 2ll * T.S) +
          (int64_t)s * T.npix;
  return g;
}

// entry of a (job, arm) in the per-arm outputs (value, status, outside, gradient rows)
// and in the cell records: arms are grid rows, the stride is the launch's J
__device__ __forceinline__ int64_t obj_out_index(int J, int j) {
  return (int64_t)blockIdx.y * J + j;
}

struct ObjArms {
  rvs_objective_arm a[RVS_MAX_ARMS];
  int n;
};

// FROMT: the unbroadened template of every (job, arm) comes from HBM -- a row
// of an evaluator that is no grid gather (the MLP of rvs_template_nn) -- with
// its outside flag; everything behind the template (FIR, spline solve, chi^2)
// is the same code.
struct ObjTempl {
  const double *templ[RVS_MAX_ARMS];    // [J, ntp] per arm
  const double *outside[RVS_MAX_ARMS];  // [J] per arm
};

// The cell search of a (job, arm) -- log10 mapping, one binary search per
// dimension, 2^ndim idgrid look-ups, weights; outside the grid the brute-force
// nearest neighbour -- is a chain of dependent loads that a few threads walk while
// the other 500 of an objective block wait: 7.7 % of the block's time on the one
// block a CU can hold.  objective_locate_kernel runs it ahead for all (job, arm)
// pairs of a launch with one wave each (thousands of them resident at once, their
// latencies overlapping) and leaves a record the objective block fetches with one
// coalesced load.  Same poly_locate code: the same ids, weights and distances.
#define OBJ_LOC_NV 16                      // grids of up to 4 dimensions
#ifndef OBJ_FIR_KMAX
#define OBJ_FIR_KMAX 8   // widest rotational kernel (half width) of the register-window FIR
#endif
// the record, in doubles (the integer fields through a cast of the record's base)
#define OBJ_LOC_W 0                         // w[OBJ_LOC_NV]: the vertex weights
#define OBJ_LOC_ID OBJ_LOC_NV               // id[OBJ_LOC_NV]: the vertex rows (int64)
#define OBJ_LOC_DIST (2 * OBJ_LOC_NV)       // distance of a point outside the grid
#define OBJ_LOC_MODE (2 * OBJ_LOC_NV + 1)   // {mode, nearest} (int32)
#define OBJ_LOC_JOBSC (2 * OBJ_LOC_NV + 2)  // {f, shift, 1 / linear step} (obj_job_scalars)
#define OBJ_LOC_ROT (2 * OBJ_LOC_NV + 5)    // {kmax, refused} of the rotational kernel (int32)
#define OBJ_LOC_TAPS (2 * OBJ_LOC_NV + 6)   // its normalised taps 0 .. kmax <= OBJ_FIR_KMAX
#define OBJ_LOC_REC (OBJ_LOC_TAPS + OBJ_FIR_KMAX + 1)

// half width of a job's rotational kernel on the arm's template grid: 0 = none (no
// rotation, or refused: `refused`), R = v sin i / c in template pixels
__device__ __forceinline__ int obj_rot_kmax(const rvs_objective_arm &T, double vs,
                                            double &R, bool &refused) {
  R = (vs / RVS_C_KMS) / T.lnstep;
  refused = false;
  if (!(vs > 0) || (R < 1e-9)) return 0;
  const int kmax = (int)ceil(R + 1);
  // (the kernel's primitives are staged in a buffer of the template's length as two
  // runs of kmax + 3 doubles: a kernel wider than that is refused like one wider than
  // the template)
  if (kmax >= T.ntp || 2 * (kmax + 3) > T.ntp) {
    refused = true;
    return 0;
  }
  return kmax;
}
// tap k (not yet normalised) from the primitives at the clipped points x_j = clip(j /
// R), j = -1 .. kmax + 1, staged as entries j + 1 of pk0 / pk1 (rot_prim)
__device__ __forceinline__ double obj_rot_tap_raw(int k, double R, const double *pk0,
                                                  const double *pk1) {
  double ww = 0;
  // x_{k-1}, x_k, x_{k+1} are entries k, k+1, k+2
  double lo = fmin(fmax(k / R, -1.0), 1.0), hi = fmin(fmax((k + 1) / R, -1.0), 1.0);
  if (hi > lo)   // rot_segment(lo, hi, -R, 1 + k)
    ww += -R * (pk1[k + 2] - pk1[k + 1]) + (1.0 + k) * (pk0[k + 2] - pk0[k + 1]);
  lo = fmin(fmax((k - 1) / R, -1.0), 1.0);
  hi = fmin(fmax(k / R, -1.0), 1.0);
  if (hi > lo)   // rot_segment(lo, hi, R, 1 - k)
    ww += R * (pk1[k + 1] - pk1[k]) + (1.0 - k) * (pk0[k + 1] - pk0[k]);
  return ww;
}
// ... and its derivative by R over the same clipped legs (vsini_kernel<true>'s W')
__device__ __forceinline__ double obj_rot_dtap_raw(int k, double R, const double *pk1) {
  double d = 0;
  double lo = fmin(fmax(k / R, -1.0), 1.0), hi = fmin(fmax((k + 1) / R, -1.0), 1.0);
  if (hi > lo) d += -1.0 * (pk1[k + 2] - pk1[k + 1]);   // rot_segment(lo, hi, -1, 0)
  lo = fmin(fmax((k - 1) / R, -1.0), 1.0);
  hi = fmin(fmax(k / R, -1.0), 1.0);
  if (hi > lo) d += 1.0 * (pk1[k + 1] - pk1[k]);        // rot_segment(lo, hi, 1, 0)
  return d;
}
// entry jj of the staged primitives: x_{jj-1} = clip((jj - 1) / R)
__device__ __forceinline__ void obj_rot_stage(int jj, double R, double eps_ld, double *pk0,
                                              double *pk1) {
  const double x = fmin(fmax((jj - 1) / R, -1.0), 1.0);
  double k0, k1;
  rot_prim(x, eps_ld, k0, k1);
  pk0[jj] = k0;
  pk1[jj] = k1;
}
// The normalisation: the kernel is symmetric, so tap k > 0 counts twice in the sum S
// of the raw taps, and a normalised tap is the raw one times 1 / S.
__device__ __forceinline__ double obj_rot_tap_mass(int k, double ww) {
  return (k == 0) ? ww : 2 * ww;
}

// The taps by the whole block of NT threads: normalised taps 0 .. kmax into wt and, with
// dwt, their derivatives by vsini (dw = (W' - w S') / S / (c lnstep)).  The primitives
// (an asin and a sqrt each, ~150 dependent fp64 instructions) are evaluated ONE per
// thread into `stage`, two runs of kmax + 3 doubles: tap k needs them at j = k-1, k,
// k+1, and evaluated inside rot_segment every tap thread walked four of them in a row
// while the other 450 threads of the block waited.  Same arguments, same function: the
// same values.  red8: NT / 64 doubles.  SUM_BARRIER: the barrier the value kernel has
// behind the sum (the gradient kernel never had it, and measured 0.6 % slower with it).
// (objective_locate_kernel has the one-wave form of the same steps for the kernels narrow
// enough for the cell record.)
template <int NT, bool SUM_BARRIER>
__device__ __forceinline__ void obj_build_taps(int kmax, double R, double eps_ld,
                                               double lnstep, double *stage, double *wt,
                                               double *dwt, double *red8) {
  const int tid = threadIdx.x;
  double *pk0 = stage, *pk1 = stage + (kmax + 3);
  for (int jj = tid; jj <= kmax + 2; jj += NT) obj_rot_stage(jj, R, eps_ld, pk0, pk1);
  __syncthreads();
  double psum = 0, dsum = 0;
  for (int k = tid; k <= kmax; k += NT) {
    const double ww = obj_rot_tap_raw(k, R, pk0, pk1);
    wt[k] = ww;
    psum += obj_rot_tap_mass(k, ww);
    if (dwt) {
      const double d = obj_rot_dtap_raw(k, R, pk1);
      dwt[k] = d;
      dsum += obj_rot_tap_mass(k, d);
    }
  }
  psum = block_sum<NT / 64>(psum, red8);
  if (dwt) dsum = block_sum<NT / 64>(dsum, red8);
  if (SUM_BARRIER) __syncthreads();
  const double inv = 1.0 / psum;
  const double dscale = inv / (RVS_C_KMS * lnstep);
  // normalised taps once (the product every output formed per tap)
  for (int k = tid; k <= kmax; k += NT) {
    const double ww = wt[k];
    if (dwt) dwt[k] = (dwt[k] - ww * inv * dsum) * dscale;
    wt[k] = ww * inv;
  }
  __syncthreads();
}

// MAX_VAL guard of getCurTempl (spec_fit.py:392-397) on a template that is a nearest
// row or an evaluator's row of a point outside its domain: a value of the row...
__device__ __forceinline__ void obj_guard_scan(double val, double &mx, bool &anynan) {
  if (!(val == val)) anynan = true;
  mx = fmax(mx, fabs(val));
}
// ... and the block's verdict from every thread's {mx, anynan}: the arm's `outside`,
// *dist (read behind the barrier) or NaN when the row is unusable.  One barrier;
// red8: 2 NW doubles.
template <int NW>
__device__ __forceinline__ double obj_template_guard(double mx, bool anynan,
                                                     const double *dist, double *red8) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  mx = wave_max(mx);
  const double nanf = wave_sum(anynan ? 1.0 : 0.0);
  if (lane == 0) {
    red8[w] = mx;
    red8[NW + w] = nanf;
  }
  __syncthreads();
  double mm = 0, nn = 0;
  for (int i = 0; i < NW; i++) {
    mm = fmax(mm, red8[i]);
    nn += red8[NW + i];
  }
  double outside = *dist;
  if (outside > 0 && (mm > 1e100 || nn > 0 || isinf(mm))) outside = __builtin_nan("");
  return outside;
}
// an arm with an unusable template is skipped: obj_sum_row charges it by its NaN
__device__ __forceinline__ bool obj_template_unusable(double outside) {
  return !(fabs(outside) <= 1.79e308);
}
__device__ __forceinline__ void obj_store_skipped(int64_t o, double *armchi, int32_t *armst,
                                                  double *armout) {
  if (threadIdx.x == 0) {
    armout[o] = __builtin_nan("");
    armchi[o] = 0.0;
    armst[o] = 0;
  }
}

// What a job's velocity turns into, the same for every pixel of the (job, arm): the
// Doppler factor f = sqrt((1 - b) / (1 + b)) (spec_fit.py:707-727), the pixels' shift in
// knot coordinates on a log-uniform grid, ln f / ln(knot ratio), or the inverse step of a
// linear one.  Two divisions, a square root and two logarithms -- ~330 instructions that
// all 512 threads of an objective block used to execute for themselves (1.3 us of the
// block's VALU issue): now ONE lane, of the cell-search kernel where it runs ahead
// (with the cell record), else of a wave that idles under the rotational kernel's
// construction.  Same expressions: same values.
__device__ __forceinline__ void obj_job_scalars(const rvs_point_arm &S, double velj,
                                                double *out) {
  const double bb = velj / RVS_C_KMS;
  const double f = sqrt((1.0 - bb) / (1.0 + bb));
  const double x0 = S.knots[0];
  out[0] = f;
  out[1] = S.log_step ? log(f) / log(S.knots[1] / x0) : 0.0;
  out[2] = S.log_step ? 0.0 : 1.0 / (S.knots[1] - x0);
}

__device__ __forceinline__ GridDesc obj_grid_desc(const rvs_objective_arm &T) {
  GridDesc G;
  const int nd = T.ndim;
  G.ndim = nd;
  G.log_mask = T.log_mask;
  int off = 0;
#pragma unroll
  for (int d = 0; d < MAXDIM; d++) {   // (static indices: the descriptor stays in registers)
    G.lens[d] = (d < nd) ? T.lens[d] : 1;
    G.uoff[d] = off;
    off += G.lens[d];
    G.ptp[d] = (d < nd) ? T.ptp[d] : 1.0;
  }
  int64_t st = 1;
#pragma unroll
  for (int d = MAXDIM - 1; d >= 0; d--) {
    if (d < nd) {
      G.gstride[d] = st;
      st *= T.lens[d];
    } else {
      G.gstride[d] = 0;
    }
  }
  return G;
}


// Wave reduction of CNT per-lane sums by halving: at the step with lane mask m the
// lanes l and l^m split the live sums between them (the lane with the bit clear
// keeps the lower half), so a step moves half as many values as the one before:
// ~CNT exchanges in all instead of CNT full butterflies.  The exchange at mask 32
// / 16 -- the upper half (odd rows) of the kept value trades places with the lower
// half (even rows) of the sent one -- IS v_permlane32_swap / v_permlane16_swap
// (gfx950), on the VALU; masks 8..1 are DPP row permutations.  (As ds_bpermute the
// exchanges of 8 waves queued on the CU's one LDS crossbar: 13.8 % of the block.)
// After the six steps slot i (< cnt) of a lane holds the wave total of sum number
// base + i when that number is < lim.
template <int CNT>
__device__ __forceinline__ void wave_halve(double (&vals)[CNT], int lane,
                                           int &cnt_o, int &base_o, int &lim_o) {
  int cnt = CNT, base = 0, lim = CNT;
#pragma unroll
  for (int mk = 32; mk >= 1; mk >>= 1) {
    const int h = (cnt + 1) >> 1;
    const bool up = (lane & mk) != 0;
#pragma unroll
    for (int i = 0; i < h; i++) {
      const bool has_hi = (i + h < cnt);
      const double lo = vals[i], hi = has_hi ? vals[i + h] : 0.0;
      if (mk >= 16) {
        const unsigned l0 = __double2loint(lo), l1 = __double2hiint(lo);
        const unsigned h0 = __double2loint(hi), h1 = __double2hiint(hi);
        if (mk == 32) {
          const auto r0 = __builtin_amdgcn_permlane32_swap(l0, h0, false, false);
          const auto r1 = __builtin_amdgcn_permlane32_swap(l1, h1, false, false);
          vals[i] = __hiloint2double(r1[0], r0[0]) + __hiloint2double(r1[1], r0[1]);
        } else {
          const auto r0 = __builtin_amdgcn_permlane16_swap(l0, h0, false, false);
          const auto r1 = __builtin_amdgcn_permlane16_swap(l1, h1, false, false);
          vals[i] = __hiloint2double(r1[0], r0[0]) + __hiloint2double(r1[1], r0[1]);
        }
      } else {
        const double send = up ? lo : hi;
        const double keep = up ? hi : lo;
        double recv;
        if (mk == 8)
          recv = dpp_get<0x141, 0xf, 0xf>(dpp_get<0x140, 0xf, 0xf>(send));
        else if (mk == 4)
          recv = dpp_get<0x1b, 0xf, 0xf>(dpp_get<0x141, 0xf, 0xf>(send));
        else if (mk == 2)
          recv = dpp_get<0x4e, 0xf, 0xf>(send);
        else
          recv = dpp_get<0xb1, 0xf, 0xf>(send);
        vals[i] = keep + recv;
      }
    }
    lim = up ? lim : min(lim, base + h);
    base += up ? h : 0;
    cnt = h;
  }
  cnt_o = cnt;
  base_o = base;
  lim_o = lim;
}


// rows [0, obj_split(P)) of the normal equations are summed in the first pass over
// the pixels: everything up to P = 10, about half of the P (P + 3) / 2 sums beyond
#ifndef OBJ_ONEPASS_MAX
#define OBJ_ONEPASS_MAX 10
#endif
__host__ __device__ constexpr int obj_split(int P) {
  if (P <= OBJ_ONEPASS_MAX) return P;
  int pa = 1;
  while (pa < P && pa * (pa + 3) < P * (P + 3) / 2) pa++;
  return pa;
}

// The hand-over between the spline's chunks.  Both sweeps of the tridiagonal solve are
// linear in the value that enters a thread's chunk of rows, d_i = d0_i + P_i d_in, so one
// pass over the chunk yields (al, be) = (d0, P) at its last row, and the value entering
// from `dir` = -1 (lower threads) or +1 (upper) is
//   d_in(t) = al(t-1) + be(t-1) (al(t-2) + be(t-2) al(t-3))
// to |be|^3 <= (0.268^12)^3 = 3e-21 (the multipliers of a (log-)uniform grid tend to
// 2 - sqrt 3; chunks hold at least 12 rows).  The three nearest chunks' coefficients come
// through wave shuffles, across a wave boundary through edge[] (static LDS; one array per
// direction: no barrier between the two uses).  One barrier.
template <int NW>
__device__ __forceinline__ double obj_chain3(double (*edge)[NW][6], double al, double be,
                                             int dir) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double (*eds)[6] = edge[dir < 0 ? 0 : 1];
  double av3[3], bv3[3];
#pragma unroll
  for (int k = 1; k <= 3; k++) {
    av3[k - 1] = (dir < 0) ? __shfl_up(al, k, 64) : __shfl_down(al, k, 64);
    bv3[k - 1] = (dir < 0) ? __shfl_up(be, k, 64) : __shfl_down(be, k, 64);
  }
  const int edge_l = (dir < 0) ? (63 - lane) : lane;   // 0..2: published lanes
  if (edge_l < 3) {
    eds[w][2 * edge_l] = al;
    eds[w][2 * edge_l + 1] = be;
  }
  __syncthreads();
  const int mine = (dir < 0) ? lane : (63 - lane);   // distance to the boundary
#pragma unroll
  for (int k = 1; k <= 3; k++) {
    if (mine < k) {   // neighbour k lives in the adjacent wave
      const int ww = w + dir;
      const int sl = k - 1 - mine;   // its distance from that wave's boundary
      const bool have = (ww >= 0 && ww < NW);
      av3[k - 1] = have ? eds[ww][2 * sl] : 0.0;
      bv3[k - 1] = have ? eds[ww][2 * sl + 1] : 0.0;
    }
  }
  return av3[0] + bv3[0] * (av3[1] + bv3[1] * av3[2]);
}

// a b rounded on its own, whatever becomes of the product: never one half of an fma
__device__ __forceinline__ double obj_mul_rounded(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}

// A pixel's knot interval (point_knot): on a log-uniform grid the pixel's knot coordinate
// plus the job's shift, on a linear one the Doppler-shifted wavelength x over the step;
// clamped to the grid's intervals.  What the job fixes is the map ...
struct ObjKnotMap {
  int log_step, N;
  double f, shift, lin_inv_step;   // obj_job_scalars
  double x0;                       // knot 0
};
// ... applied to a pixel whose terms are at hand (x = lam f) ...
__device__ __forceinline__ int obj_knot_interval(const ObjKnotMap &K, double pixc, double x) {
  const int pos = K.log_step ? (int)(pixc + K.shift) : (int)((x - K.x0) * K.lin_inv_step);
  return min(max(pos, 0), K.N - 2);
}
// ... or to pixel k of the arm's tables (which loads the one term its grid needs)
__device__ __forceinline__ int obj_knot_interval(const ObjKnotMap &K, const ObjArmGrid &AG,
                                                 int k) {
  return K.log_step ? obj_knot_interval(K, AG.pix[k], 0.0)
                    : obj_knot_interval(K, 0.0, AG.lam[k] * K.f);
}

// Spline piece of interval pos in powers of dl = x - x_pos, exactly as
// rvs_spline_construct(form 1) stores it: y the template's values at the knots, z[u] the
// second derivative at knot u + 1 (natural ends), h / hinv the interval's width and its
// reciprocal.
struct ObjPiece {
  double yi, cb, c2, c3;
};
__device__ __forceinline__ ObjPiece obj_piece(int pos, int N, double h, double hinv,
                                              const double *y, const double *z) {
  ObjPiece p;
  const double zi = (pos == 0) ? 0.0 : z[pos - 1];
  const double zi1 = (pos + 1 == N - 1) ? 0.0 : z[pos];
  const double yi1 = y[pos + 1];
  p.yi = y[pos];
  const double t1 = hinv * (1.0 / 6), t2 = h * (1.0 / 6);
  p.cb = (yi1 - p.yi) * hinv - t2 * (2 * zi + zi1);
  p.c2 = 0.5 * zi;
  p.c3 = (zi1 - zi) * t1;
  return p;
}
__device__ __forceinline__ double obj_piece_value(const ObjPiece &p, double dl) {
  return fma(fma(fma(p.c3, dl, p.c2), dl, p.cb), dl, p.yi);
}
__device__ __forceinline__ double obj_piece_deriv(const ObjPiece &p, double dl) {
  return fma(dl, fma(3.0 * p.c3, dl, 2.0 * p.c2), p.cb);
}

// Value and status of a (job, arm) as rvs_chisq_point forms them: ldet = log det L, ok =
// every pivot positive, rr = the residual norm; the spectrum's pixels must lie on the
// template's knots [x0, xlast) at the job's velocity.
__device__ __forceinline__ void obj_value_status(const rvs_point_arm &S, const ObjArmGrid &AG,
                                                 int s, const ObjKnotMap &K, double xlast,
                                                 double ldet, bool ok, double rr,
                                                 int st_extra, double &chi, int &st) {
  const double lz = AG.wbase[2ll * S.S * S.npix + 2 * s];
  chi = 2.0 * ldet + 2.0 * lz + rr;
  st = st_extra;
  const double xa = AG.lam[0] * K.f, xb = AG.lam[S.npix - 1] * K.f;
  if (xa < K.x0 || xb < K.x0 || xa >= xlast || xb >= xlast) {
    st |= RVS_ST_SPLINE_RANGE;
    chi = __builtin_nan("");
  }
  if (!ok) st |= RVS_ST_CHOL_FALLBACK;
  if (!ok || !(fabs(chi) <= 1.79e308)) {
    st |= RVS_ST_NONFINITE;
    chi = __builtin_nan("");
  }
}
