// Validation metrics on the device (MAE / RMSE in mm, iMAE / iRMSE in 1/km): the per-sample block of validate() and run()
// (src/fusionnet_main.py:528-548, :826-843 with src/eval_utils.py) as a two-stage, fixed-order fp64 reduction.
//
// Stage 1, eval_partial_kernel: grid (blocks per sample, n).  A sample's pixels are cut into chunks of EVAL_CHUNK; block b of a
// sample takes the chunks b, b + blocks, ... and inside a chunk thread t owns the quads t, t + 256, ... -- which pixel is summed by
// which thread, and in which order, depends on `pix` alone.  Neither the batch size, nor the sample's position, nor the load path
// (16-byte loads when both sample bases are 16-byte aligned, scalar loads otherwise and for the last 1-3 pixels) changes one bit.
// Every block leaves 5 doubles (sum |e|, sum e^2, sum |ie|, sum ie^2, count) in its own workspace slot: wave shuffles -> LDS -> one
// store per value.  Stage 2, eval_final_kernel: one block; each wave sums the slots of one sample at a time in a fixed order, takes
// the means and square roots and writes row cursor[0] + s of `results`; thread 0 then advances the cursor.  No atomics anywhere.
#include "rcf_common.h"

#define EVAL_THREADS 256
#define EVAL_CHUNK 4096          // pixels per chunk: 4 quads per thread
#define EVAL_FINAL_THREADS 1024

#pragma clang fp contract(off)   // (a*b + c stays two roundings: the result is a property of the inputs, not of the compiler's fusing)

struct EvalAcc { double ae, se, iae, ise; int cnt; };

__device__ __forceinline__ void eval_pixel(EvalAcc& a, float g, float o, float lo, float hi) {
    if (g > 0.f && g > lo && g < hi) {        // fp32 comparisons, as numpy compares a float32 array with a Python scalar
        const double gd = (double)g, od = (double)o;
        const double e = 1000.0 * gd - 1000.0 * od;
        const double ie = 1.0 / (0.001 * gd) - 1.0 / (0.001 * od);
        a.ae += fabs(e);
        a.se += e * e;
        a.iae += fabs(ie);
        a.ise += ie * ie;
        a.cnt += 1;
    }
}

__global__ void __launch_bounds__(EVAL_THREADS) eval_partial_kernel(const float* __restrict__ depth, const float* __restrict__ gt,
                                                                    long long pix, float lo, float hi, double* __restrict__ ws) {
    __shared__ double sm[EVAL_THREADS / 64][5];
    const int s = blockIdx.y;
    const float* __restrict__ o = depth + (size_t)s * (size_t)pix;
    const float* __restrict__ g = gt + (size_t)s * (size_t)pix;
    const bool aligned = (((uintptr_t)o | (uintptr_t)g) & 15u) == 0;    // uniform over the block
    const long long n_chunk = (pix + EVAL_CHUNK - 1) / EVAL_CHUNK;
    EvalAcc a = {0.0, 0.0, 0.0, 0.0, 0};
    for (long long c = blockIdx.x; c < n_chunk; c += gridDim.x) {
#pragma unroll
        for (int j = 0; j < EVAL_CHUNK / (4 * EVAL_THREADS); ++j) {
            const long long i = c * EVAL_CHUNK + (long long)(j * EVAL_THREADS + threadIdx.x) * 4;
            if (i >= pix) continue;
            if (aligned && i + 3 < pix) {
                const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
                const f32x4 ov = *reinterpret_cast<const f32x4*>(o + i);
#pragma unroll
                for (int k = 0; k < 4; ++k) eval_pixel(a, gv[k], ov[k], lo, hi);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (i + k < pix) eval_pixel(a, g[i + k], o[i + k], lo, hi);
            }
        }
    }
    double v[5] = {a.ae, a.se, a.iae, a.ise, (double)a.cnt};
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[q] += __shfl_xor(v[q], off);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q < 5; ++q) sm[wave][q] = v[q];
    __syncthreads();
    if (threadIdx.x < 5) {
        const int q = threadIdx.x;
        ws[((size_t)s * 5 + q) * RCF_EVAL_BLOCKS + blockIdx.x] = ((sm[0][q] + sm[1][q]) + sm[2][q]) + sm[3][q];
    }
}

__global__ void __launch_bounds__(EVAL_FINAL_THREADS) eval_final_kernel(const double* __restrict__ ws, int n, int blocks,
                                                                        double* __restrict__ results, int capacity,
                                                                        int* __restrict__ cursor) {
    const int base = cursor[0];
    __syncthreads();                              // every thread holds the row index before thread 0 moves it
    const bool fits = base >= 0 && (long long)base + n <= (long long)capacity;
    if (fits) {
        const int lane = threadIdx.x & 63;
        for (int s = threadIdx.x >> 6; s < n; s += EVAL_FINAL_THREADS / 64) {
            double v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const double* __restrict__ row = ws + ((size_t)s * 5 + q) * RCF_EVAL_BLOCKS;
                double t = 0.0;
                for (int b = lane; b < blocks; b += 64) t += row[b];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
                v[q] = t;
            }
            if (lane == 0) {
                double* __restrict__ r = results + (size_t)(base + s) * 5;
                const double cnt = v[4];          // 0 pixels: 0 / 0 = NaN in all four, as np.mean of an empty array
                r[0] = v[0] / cnt;
                r[1] = sqrt(v[1] / cnt);
                r[2] = v[2] / cnt;
                r[3] = sqrt(v[3] / cnt);
                r[4] = cnt;
            }
        }
    }
    if (threadIdx.x == 0) {
        if (fits) cursor[0] = base + n;
        else cursor[1] += n;
    }
}

static inline int eval_blocks(long long pix) {
    const long long n_chunk = (pix + EVAL_CHUNK - 1) / EVAL_CHUNK;
    return (int)(n_chunk < RCF_EVAL_BLOCKS ? n_chunk : RCF_EVAL_BLOCKS);
}

extern "C" int rcf_eval_metrics(const float* depth, const float* ground_truth, int n, long long pix, float min_evaluate_depth,
                                float max_evaluate_depth, double* workspace, double* results, int capacity, int* cursor, void* stream) {
    if (!depth || !ground_truth || !workspace || !results || !cursor || n <= 0 || n > 65535 || pix <= 0 || capacity <= 0) return RCF_EINVAL;
    const int blocks = eval_blocks(pix);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_partial_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(EVAL_THREADS), 0, st, depth, ground_truth, pix,
                       min_evaluate_depth, max_evaluate_depth, workspace);
    int rc = rcf_launch_status();
    if (rc != RCF_OK) return rc;
    hipLaunchKernelGGL(eval_final_kernel, dim3(1), dim3(EVAL_FINAL_THREADS), 0, st, workspace, n, blocks, results, capacity, cursor);
    return rcf_launch_status();
}
