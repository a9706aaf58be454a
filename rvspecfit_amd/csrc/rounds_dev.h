// rounds_dev.h -- the rounds of the machines whose runs live on the device, stated once
// (bfgs_dev.hip: rvs_bfgs_run, rvs_bfgs_run_grad*; lm_dev.hip: rvs_lm_run*):
//   rounds_scan_kernel  exclusive scan of the row counts: every run's first row, the
//                       rows of each launch chunk, the number of live runs
//   rounds_emit_kernel  the requested points into one list (run order)
//   rounds_fill         the fields every machine's descriptor shares, from its state
//   rounds_run          the round driver: advance -> scan -> emit -> the objective per
//                       chunk of `cap` rows, the host's looks at the counts, the result
// `Dev` is the machine's descriptor: S, n, cap, nreq, off, list, counts, X, F and runs,
// with rounds_request_rows(run) the run's pending rows [nreq, n].
#pragma once
#include "common.h"

#define BF_SCAN_NT 1024
#define BF_NCHUNK 24    // counts[0 .. 24): rows of chunk c; [24] rows; [25] live runs

template <class Dev>
__global__ void __launch_bounds__(BF_SCAN_NT) rounds_scan_kernel(Dev D) {
  __shared__ int wsum[BF_SCAN_NT / 64];
  __shared__ int carry[2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry[0] = carry[1] = 0;
  __syncthreads();
  for (int s0 = 0; s0 < D.S; s0 += BF_SCAN_NT) {
    const int s = s0 + tid;
    const int nr = (s < D.S) ? D.nreq[s] : 0;
    int v = nr;   // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o, 64);
      if (lane >= o) v += t;
    }
    if (lane == 63) wsum[w] = v;
    const int alive = wave_sum_i(nr > 0 ? 1 : 0);
    __syncthreads();
    int base = carry[0];
    for (int i = 0; i < w; i++) base += wsum[i];
    if (s < D.S) D.off[s] = base + v - nr;
    __syncthreads();
    if (lane == 0 && alive) atomicAdd(&carry[1], alive);
    if (tid == BF_SCAN_NT - 1) carry[0] = base + v;
    __syncthreads();
  }
  if (tid < BF_NCHUNK) {
    const int rest = carry[0] - tid * D.cap;
    D.counts[tid] = rest < 0 ? 0 : (rest > D.cap ? D.cap : rest);
  }
  if (tid == 0) {
    D.counts[BF_NCHUNK] = carry[0];
    D.counts[BF_NCHUNK + 1] = carry[1];
  }
}

template <class Dev>
__global__ void __launch_bounds__(256) rounds_emit_kernel(Dev D) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int per = D.n + 1;
  const int s = t / per, q = t - s * per;
  if (s >= D.S || q >= D.nreq[s]) return;
  const int j = D.off[s] + q, n = D.n;
  D.list[j] = s;
  const double *src = rounds_request_rows(D.runs[s]) + q * n;
  for (int i = 0; i < n; i++) D.X[(int64_t)j * n + i] = src[i];
}

template <class Dev, class State, class R>
void rounds_fill(Dev &D, const State *b, R *runs, int cap) {
  D.runs = runs;
  D.S = b->S, D.n = b->n, D.cap = cap;
  D.nreq = b->nreq, D.off = b->off, D.list = b->list, D.counts = b->counts;
  D.X = b->X, D.F = b->F;
}

// The rounds of S runs until every run is done.  advance(first, stream) launches the
// machine's advance kernel (first = 1: start the runs); eval(list, X, J, chunk, F, stream)
// answers a chunk of J rows into F [J, width]; result(stream) launches the kernel or
// kernels that write the results.  `behind`: the rows a live run may ask for in a round
// the host does not look at (S * behind rows bound every round).  stats: rounds, eval
// calls, rows launched.
// The counts stay on the device: the host looks (a 128-byte copy) every round while the
// launches are large, so that every chunk launched has rows; in the tail every sync_every
// rounds, behind the bound "every live run asks for `behind` rows" -- the rows behind the
// device count cost next to nothing -- and only to bound the launches and to see the end:
// a run's path does not depend on when it looks.
template <class Dev, class Advance, class Eval, class Result>
int rounds_run(const Dev &D, int behind, int width, int sync_every, int64_t *stats,
               void *stream, Advance advance, Eval eval, Result result) {
  const int n = D.n, cap = D.cap;
  const int64_t maxrows = (int64_t)D.S * behind;
  if (cap < 1 || (maxrows + cap - 1) / cap > BF_NCHUNK) return RVS_E_ARG;
  hipStream_t st = rvs_stream(stream);
  const dim3 egrid((int)(((int64_t)D.S * (n + 1) + 255) / 256));
  auto step = [&](int first) {
    advance(first, st);
    hipLaunchKernelGGL(rounds_scan_kernel<Dev>, dim3(1), dim3(BF_SCAN_NT), 0, st, D);
    hipLaunchKernelGGL(rounds_emit_kernel<Dev>, egrid, dim3(256), 0, st, D);
  };
  step(1);
  RVS_LAUNCH_CHECK();
  int64_t rounds = 0, calls = 0, jobs = 0;
  int32_t c[BF_NCHUNK + 8];
  while (true) {
    if (hipMemcpyAsync(c, D.counts, sizeof(int32_t) * (BF_NCHUNK + 2),
                       hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return RVS_E_LAUNCH;
    const int64_t total = c[BF_NCHUNK], live = c[BF_NCHUNK + 1];
    if (total == 0) break;
    const int window = (total > 4096) ? 1 : sync_every;
    for (int r = 0; r < window; r++) {
      int64_t bound = (r == 0) ? total : live * behind;
      if (bound > maxrows) bound = maxrows;
      for (int64_t a = 0, ch = 0; a < bound; a += cap, ch++) {
        const int J = (int)((bound - a < cap) ? bound - a : cap);
        int rc = eval(D.list + a, D.X + a * n, J, (int)ch, D.F + a * width, st);
        if (rc) return rc;
        calls++;
        jobs += J;
      }
      step(0);
      RVS_LAUNCH_CHECK();
      rounds++;
    }
  }
  result(st);
  RVS_LAUNCH_CHECK();
  if (hipStreamSynchronize(st) != hipSuccess) return RVS_E_LAUNCH;
  if (stats) {
    stats[0] = rounds;
    stats[1] = calls;
    stats[2] = jobs;
  }
  return 0;
}
