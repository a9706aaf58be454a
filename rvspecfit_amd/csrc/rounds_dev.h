// rounds_dev.h -- the two kernels between the advance of a round and its objective,
// stated once for the machines whose runs live on the device (bfgs_dev.hip: rvs_bfgs_run,
// rvs_bfgs_run_grad; lm_dev.hip: rvs_lm_run):
//   rounds_scan_kernel  exclusive scan of the row counts: every run's first row, the
//                       rows of each launch chunk, the number of live runs
//   rounds_emit_kernel  the requested points into one list (run order)
// `Dev` is the machine's descriptor: S, n, cap, nreq, off, list, counts, X and runs, with
// rounds_request_rows(run) the run's pending rows [nreq, n].
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
