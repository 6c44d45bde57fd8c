// Small streaming kernels of the train step: fused Adam over the flat parameter buffer, and the per-step re-layout of
// the f32 master weights (kept in the reference's state_dict shapes) into the storage-dtype GEMM operand layouts.
#include "cpc_common.h"
#include "cpc_kernels.h"
#include <algorithm>
#include <cstdlib>

namespace {

// Conv weight W[co][c][tap] (f32, reference layout) ->
//   fwd  [co][(j, c)]            : gemm_nt Bt operand of the forward conv       (K = kw * Cin)
//   dgrd [(r, c)][(dd, co)]      : gemm_nt Bt operand of the data gradient      (K = D * Cout), tap = r + (D-1-dd)*stride,
//                                  zero where tap >= kw.  D = ceil(kw / stride).
// A workgroup takes a 32 (co) x 32 (c) x kw tile through LDS: W is read along (c, tap) — contiguous — and both layouts are written
// in 64-byte runs (32 c of one (co, j); 32 co of one (r, c, dd)).  The element-per-thread form (4-byte gathers at a stride of kw
// floats, 2 048 workgroups) ran 50-100 us per layer on the side stream beside the backward GEMMs.
template <typename T>
__device__ __forceinline__ void conv_w_prep_tile(const float* __restrict__ W, T* __restrict__ fwd, T* __restrict__ dgrd, int Cout, int Cin,
                                                 int kw, int stride, int D, int tco, int bx, int by, float* tile) {
    const int rs = 32 * kw + 1;                        // tile [tco][32 * kw + 1], tco = 32 (a smaller power of two for very wide kernels: LDS)
    const int c0 = bx * 32, co0 = by * tco;
    const int tid = threadIdx.x;
    const int nc = min(32, Cin - c0), nco = min(tco, Cout - co0);
    for (int i = tid; i < tco * 32 * kw; i += 256) {
        const int col = i / (32 * kw), rem = i % (32 * kw);          // rem = cl * kw + tap: contiguous in W for one co
        float v = 0.f;
        if (col < nco && rem < nc * kw) v = W[((long long)(co0 + col) * Cin + c0) * kw + rem];
        tile[col * rs + rem] = v;
    }
    __syncthreads();
    if (fwd) {
        for (int i = tid; i < tco * kw * 32; i += 256) {
            const int cl = i % 32, j = (i / 32) % kw, col = i / (32 * kw);
            if (col < nco && cl < nc) fwd[((long long)(co0 + col) * kw + j) * Cin + c0 + cl] = from_f32<T>(tile[col * rs + cl * kw + j]);
        }
    }
    if (dgrd) {
        for (int i = tid; i < stride * 32 * D * tco; i += 256) {
            const int col = i % tco, dd = (i / tco) % D, cl = (i / (tco * D)) % 32, r = i / (tco * D * 32);
            const int tap = r + (D - 1 - dd) * stride;
            if (col < nco && cl < nc)
                dgrd[(((long long)r * Cin + c0 + cl) * D + dd) * Cout + co0 + col] = from_f32<T>(tap < kw ? tile[col * rs + cl * kw + tap] : 0.f);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void conv_w_prep_kernel(const float* __restrict__ W, T* __restrict__ fwd,
                                                          T* __restrict__ dgrd, int Cout, int Cin, int kw, int stride, int D, int tco) {
    extern __shared__ float tile[];
    conv_w_prep_tile<T>(W, fwd, dgrd, Cout, Cin, kw, stride, D, tco, blockIdx.x, blockIdx.y, tile);
}

// The same for a list of convolutions in ONE launch (a context network's eleven kernels of 5 x 512 x 512 took eleven launches of 20 us on
// the queue in front of the step).  jobs[j] (device) = {W, fwd, dgrd, Cout, Cin, kw, stride, D, tco, gx, first}: the job's workgroups are
// [first, first + gx * gy) of the grid, (bx, by) = (local % gx, local / gx).
struct ConvPrepJob { const float* W; void* fwd; void* dgrd; int Cout, Cin, kw, stride, D, tco, gx, first; };
template <typename T>
__global__ __launch_bounds__(256) void conv_w_prep_batch_kernel(const ConvPrepJob* __restrict__ jobs, int njobs) {
    extern __shared__ float tile[];
    int j = 0;
    while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].first) ++j;
    const ConvPrepJob q = jobs[j];
    const int local = blockIdx.x - q.first;
    conv_w_prep_tile<T>(q.W, (T*)q.fwd, (T*)q.dgrd, q.Cout, q.Cin, q.kw, q.stride, q.D, q.tco, local % q.gx, local / q.gx, tile);
}

// dst[r][c] = (T) src[r * sr + c * sc]   (dst contiguous [R][C])
template <typename T>
__global__ __launch_bounds__(256) void cast2d_kernel(const float* __restrict__ src, T* __restrict__ dst, int R, int C,
                                                     long long sr, long long sc) {
    const long long total = (long long)R * C;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int c = (int)(idx % C);
        const long long r = idx / C;
        dst[idx] = from_f32<T>(src[r * sr + (long long)c * sc]);
    }
}

// The same through a 32 x 32 LDS tile: the source is read along whichever of its axes has unit stride (sc == 1: rows; otherwise along r,
// e.g. the transposed copy sr == 1), the destination is written along c.  One element per thread and iteration in cast2d_kernel with
// 64-bit div / mod and — for a transposed copy — a 4-byte read per 2 KiB of stride: 21 - 30 us for the 0.4 M elements of a GRU input
// projection; the tile form is bound by the launch.
template <typename T>
__global__ __launch_bounds__(256) void cast2d_tile_kernel(const float* __restrict__ src, T* __restrict__ dst, int R, int C, long long sr,
                                                          long long sc) {
    __shared__ float t[32][33];
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (sc == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = r0 + ty + 8 * k, c = c0 + tx;
            t[ty + 8 * k][tx] = (r < R && c < C) ? src[(long long)r * sr + c] : 0.f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + ty + 8 * k, r = r0 + tx;
            t[tx][ty + 8 * k] = (r < R && c < C) ? src[(long long)r * sr + (long long)c * sc] : 0.f;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + ty + 8 * k, c = c0 + tx;
        if (r < R && c < C) dst[(long long)r * C + c] = from_f32<T>(t[ty + 8 * k][tx]);
    }
}

// Many cast2d jobs in one launch (the operand-layout copies of a context network: 26 small matrices for a 3-layer transformer):
// jobs[y] = {src, dst, R, C, sr, sc}, all 64-bit, in device memory; grid (x, number of jobs).
struct CastJob { const float* src; void* dst; long long R, C, sr, sc; };
template <typename T>
__global__ __launch_bounds__(256) void cast2d_batch_kernel(const CastJob* __restrict__ jobs) {
    const CastJob j = jobs[blockIdx.y];
    T* dst = (T*)j.dst;
    const long long total = j.R * j.C;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long c = idx % j.C, r = idx / j.C;
        dst[idx] = from_f32<T>(j.src[r * j.sr + c * j.sc]);
    }
}

// MaxPool1d(pool, ceil_mode=True) over positions of a channels-last activation (ConvolutionalArBlock, audio_model.py:98-99).
// out[b][p][c] = max_{i < pool, p*pool+i < Lin_valid} in[b][p*pool+i][c];  pad rows (p >= Lout_valid) get zeros.  A NaN in a window
// is its maximum, as in torch (a window element replaces the running maximum when it is greater or NaN): the NaN guard of the
// training loop must see it.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ in, T* __restrict__ out, int B, int C, int pool,
                                                          int Lin_valid, int Lin_alloc, int Lout_valid, int Lout_alloc) {
    const int c4n = C / 4;
    const long long total = (long long)B * Lout_alloc * c4n;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int c4 = (int)(idx % c4n);
        const int pp = (int)((idx / c4n) % Lout_alloc);
        const int b = (int)(idx / ((long long)c4n * Lout_alloc));
        f32x4 m = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (pp < Lout_valid) {
            const T* src = in + ((long long)b * Lin_alloc + (long long)pp * pool) * C + c4 * 4;
            m = load4(src);
            for (int i = 1; i < pool && pp * pool + i < Lin_valid; ++i) {
                const f32x4 v = load4(src + (long long)i * C);
#pragma unroll
                for (int e = 0; e < 4; ++e) m[e] = (v[e] > m[e] || v[e] != v[e]) ? v[e] : m[e];
            }
        }
        store4(out + ((long long)b * Lout_alloc + pp) * C + c4 * 4, m);
    }
}

// Backward of the pooling: the gradient of a window goes to the element the forward rule above ends on (torch semantics): the
// FIRST maximal element, or the LAST NaN of a window holding NaN; everything else, and the pad rows, get zeros.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ in, const T* __restrict__ dout, T* __restrict__ din,
                                                          int B, int C, int pool, int Lin_valid, int Lin_alloc, int Lout_alloc) {
    const int c4n = C / 4;
    const long long total = (long long)B * Lin_alloc * c4n;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int c4 = (int)(idx % c4n);
        const int x = (int)((idx / c4n) % Lin_alloc);
        const int b = (int)(idx / ((long long)c4n * Lin_alloc));
        f32x4 g = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (x < Lin_valid) {
            const int pp = x / pool, me = x % pool;
            const T* src = in + ((long long)b * Lin_alloc + (long long)pp * pool) * C + c4 * 4;
            const f32x4 d = load4(dout + ((long long)b * Lout_alloc + pp) * C + c4 * 4);
            f32x4 best = load4(src);
            int arg[4] = {0, 0, 0, 0};
            for (int i = 1; i < pool && pp * pool + i < Lin_valid; ++i) {
                const f32x4 v = load4(src + (long long)i * C);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; arg[e] = i; }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = arg[e] == me ? d[e] : 0.f;
        }
        store4(din + ((long long)b * Lin_alloc + x) * C + c4 * 4, g);
    }
}

// dy[b][row][c] = y[b][row][c] > 0 ? dc[b][c] : 0   (gradient entering the last ReLU of the conv context network at the one
// position ConvolutionalArModel.forward returns, audio_model.py:161); dy is otherwise left untouched.
template <typename T>
__global__ __launch_bounds__(256) void relu_row_bwd_kernel(const float* __restrict__ dc, const T* __restrict__ y, T* __restrict__ dy,
                                                           int B, int C, long long item_stride, long long row_off) {
    const int total = B * C;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int b = idx / C, c = idx % C;
        const long long o = (long long)b * item_stride + row_off + c;
        dy[o] = from_f32<T>(to_f32(y[o]) > 0.f ? dc[idx] : 0.f);
    }
}

}  // namespace

// ---- gradient clipping by global norm (torch.nn.utils.clip_grad_norm_; include/cpc_hip.h, cpc_grad_norm / cpc_adam_clip) ----
// Stage 1: a workgroup takes GN_TILE = 256 threads x GN_CHAIN 16-byte loads = 8 192 consecutive floats; thread t reads the float4s
// t, t + 256, ... of the tile (contiguous over the wave) and keeps four f32 chains acc[e] = fma(x, x, acc[e]) of GN_CHAIN links each,
// x = g * grad_scale; then (acc0 + acc1) + (acc2 + acc3); thread t < n % 4 of the LAST workgroup adds the square of scalar-tail
// element t; an xor-shuffle tree over the wave (6 levels), (w0 + w1) + (w2 + w3) over the four waves, one partial per workgroup.
// Stage 2 (one workgroup): thread t adds the partials t, t + 256, ... in that order, then the same wave and workgroup tree.
// Every sum has a fixed shape, there is no atomic: the same data give the same bits.  Roundings on the longest path from an
// element to the total (tests/test_grad_clip_gpu.py computes its bound from these numbers):
//   2 (the scaled value, squared) + GN_CHAIN + 2 + 1 (tail) + 6 + 2   +   ceil(workgroups / 256) + 6 + 2.
constexpr int GN_CHAIN = 8;
constexpr long long GN_TILE4 = 256LL * GN_CHAIN;          // float4s per workgroup

__device__ __forceinline__ float gn_block_sum(float s, float* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ g, long long n, float grad_scale,
                                                                float* __restrict__ partial) {
    __shared__ float lds[4];
    const long long n4 = n / 4;
    const long long base = (long long)blockIdx.x * GN_TILE4 + threadIdx.x;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    if ((long long)(blockIdx.x + 1) * GN_TILE4 <= n4) {          // whole tile: GN_CHAIN independent loads in flight
        f32x4 x[GN_CHAIN];
#pragma unroll
        for (int c = 0; c < GN_CHAIN; ++c) x[c] = ((const f32x4*)g)[base + c * 256];
#pragma unroll
        for (int c = 0; c < GN_CHAIN; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xe = x[c][e] * grad_scale;
                acc[e] = __builtin_fmaf(xe, xe, acc[e]);
            }
    } else {
        for (int c = 0; c < GN_CHAIN; ++c) {
            const long long i = base + c * 256;
            if (i >= n4) break;
            const f32x4 x = ((const f32x4*)g)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xe = x[e] * grad_scale;
                acc[e] = __builtin_fmaf(xe, xe, acc[e]);
            }
        }
    }
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    if (blockIdx.x == gridDim.x - 1 && n4 * 4 + threadIdx.x < n) {          // scalar tail: at most three elements
        const float xe = g[n4 * 4 + threadIdx.x] * grad_scale;
        s = __builtin_fmaf(xe, xe, s);
    }
    s = gn_block_sum(s, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// state[0] = norm, state[1] = clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)), state[2] = 1 if the norm is NaN or inf
// (then state[1] = 0 and nan_pair, when given, is raised: the NaN guard's step indicator and sticky flag), state[3] = max_norm
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const float* __restrict__ partial, int nparts, float max_norm,
                                                              float* __restrict__ state, float* __restrict__ nan_pair) {
    __shared__ float lds[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += partial[i];
    s = gn_block_sum(s, lds);
    if (threadIdx.x != 0) return;
    const float norm = sqrtf(s);
    const bool bad = !(fabsf(norm) <= 3.402823466e38f);          // NaN or inf
    state[0] = norm;
    state[1] = bad ? 0.f : fminf(1.f, max_norm / (norm + 1e-6f));
    state[2] = bad ? 1.f : 0.f;
    state[3] = max_norm;
    if (bad && nan_pair) { nan_pair[0] = 1.f; nan_pair[1] = 1.f; }
}

long long grad_norm_workspace_floats(long long n) {
    if (n <= 0) return 0;
    return std::max(1LL, (n / 4 + GN_TILE4 - 1) / GN_TILE4);          // one partial per workgroup
}

int launch_grad_norm(const float* g, long long n, float grad_scale, float max_norm, float* workspace, float* state, float* nan_pair,
                     hipStream_t stream) {
    if (n <= 0 || !g || ((uintptr_t)g % 16) || !workspace || !state || !(max_norm > 0.f) || !(max_norm <= 3.402823466e38f))
        return CPC_EINVAL;
    const long long blocks = grad_norm_workspace_floats(n);
    if (blocks > 0x7fffffffLL) return CPC_EINVAL;
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g, n, grad_scale, workspace);
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, stream, (const float*)workspace, (int)blocks, max_norm, state,
                       nan_pair);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// ---- the learning-rate schedule (torch.optim.lr_scheduler.LambdaLR; include/cpc_hip.h, cpc_lr_factors / cpc_adamw_dev) ----
// LRSchedule.factor(s) of engine.py in double: s is the 0-based index of the step, kind 0 constant / 1 linear / 2 cosine.
__device__ __forceinline__ double lr_factor(int kind, long long warmup, long long total, double min_ratio, long long s) {
    if (s < warmup) return (double)(s + 1) / (double)warmup;
    if (kind == 0) return 1.0;
    const double q = fmin((double)(s - warmup) / (double)(total - warmup), 1.0);
    if (kind == 1) return min_ratio + (1.0 - min_ratio) * (1.0 - q);
    return min_ratio + (1.0 - min_ratio) * 0.5 * (1.0 + cos(3.14159265358979323846 * q));
}

__global__ void lr_factors_kernel(int kind, long long warmup, long long total, float min_ratio, long long step0, int count,
                                  float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = (float)lr_factor(kind, warmup, total, (double)min_ratio, step0 + i);
}

static bool lr_schedule_ok(int kind, long long warmup, long long total, float min_ratio) {
    if (kind < 0 || kind > 2 || warmup < 0 || !(min_ratio >= 0.f && min_ratio <= 1.f)) return false;
    return kind == 0 || total > warmup;
}

int launch_lr_factors(int kind, long long warmup_steps, long long total_steps, float min_ratio, long long step0, int count, float* out,
                      hipStream_t stream) {
    if (!lr_schedule_ok(kind, warmup_steps, total_steps, min_ratio) || step0 < 0 || count <= 0 || !out) return CPC_EINVAL;
    hipLaunchKernelGGL(lr_factors_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, kind, warmup_steps, total_steps, min_ratio,
                       step0, count, out);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// ---- Adam / AdamW (include/cpc_hip.h: cpc_adam, cpc_adam_clip, cpc_adamw, cpc_adam_dev, cpc_adamw_dev) ----
// torch.optim.Adam (no amsgrad):  m = m + (g - m)(1 - b1);  v = b2 v + (1 - b2) g^2;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),
// with g pre-multiplied by grad_scale (1 / world size for DP means) and, for torch.optim.AdamW, p <- p (1 - lr wd) in front.
// The scalars of one step: step_size = lr / (1 - b1^t), inv_bc2_sqrt = 1 / sqrt(1 - b2^t), decay = 1 - lr wd, cf = clipping coefficient.
struct AdamStep { float step_size, inv_bc2_sqrt, decay, b1, b2, eps, grad_scale, cf; };

// The update of one element, the only copy of it: all five entry points give the same bits because they run this text.
// COEF: the gradient is (g * grad_scale) * cf, in that order (cf == 1 is exact), otherwise g * grad_scale, which the compiler contracts
// into the first-moment update — a compile-time choice, so that neither form changes the other's roundings.  DECAY: the decay is a
// select in front of the update (never an operand of its subtraction), so that an undecayed element keeps the plain update's bits.
template <bool COEF, bool DECAY>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, bool dec, const AdamStep& k) {
    const float pd = (DECAY && dec) ? p * k.decay : p;
    float ge = g * k.grad_scale;
    if (COEF) ge = ge * k.cf;
    m = m + (ge - m) * (1.f - k.b1);
    v = v * k.b2 + (1.f - k.b2) * ge * ge;
    p = pd - k.step_size * (m / (sqrtf(v) * k.inv_bc2_sqrt + k.eps));
}

// bit blk % 32 of word blk / 32: does the 64-float block blk of the flat buffer decay?
__device__ __forceinline__ bool decay_bit(const unsigned* __restrict__ bits, long long blk) {
    return (bits[blk >> 5] >> (unsigned)(blk & 31)) & 1u;
}

// The one streaming kernel of the five entry points: <false, false> is cpc_adam's and carries no bitmap load and no select, COEF reads
// the coefficient from coef[0], DECAY the bitmap (p points at block first_block).  With ``state`` the step scalars come from the device
// (adam_tick_kernel), otherwise from the arguments.  (The scalars are separate kernel arguments, not an AdamStep: with the struct as
// the argument the compiler pairs the tail's products differently and rounds its second moment another way.)
template <bool COEF, bool DECAY>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long long n, float step_size, float b1, float b2, float eps,
                                                   float inv_bc2_sqrt, float grad_scale, float decay, const float* __restrict__ state,
                                                   const float* __restrict__ coef, const unsigned* __restrict__ bits,
                                                   long long first_block, const float* __restrict__ skip) {
    // NaN guard (contrastive_estimation_training.py:124-133 returns BEFORE backward() / optimizer.step()): the loss kernel raises
    // *skip when the loss is NaN and this update becomes a no-op — parameters and moments keep their last good values
    if (skip && skip[0] != 0.f) return;
    AdamStep k = {step_size, inv_bc2_sqrt, decay, b1, b2, eps, grad_scale, 1.f};
    if (state) { k.step_size = state[1]; k.inv_bc2_sqrt = state[2]; if (DECAY) k.decay = state[3]; }
    if (COEF) k.cf = coef[0];
    const long long n4 = n / 4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        // a float4 lies inside one 64-float block: 16 consecutive lanes share the bitmap word (one cached 4-byte load)
        const bool dec = DECAY ? decay_bit(bits, first_block + (i >> 4)) : false;
        // gradient and moments are touched once per step: non-temporal, so that 130 MB of them per step do not push the activations and
        // gradients the backward GEMMs are working on out of the Infinity Cache (the parameters are read again by the layout kernels)
        f32x4 pp = ((f32x4*)p)[i], gg = __builtin_nontemporal_load((const f32x4*)g + i), mm = __builtin_nontemporal_load((f32x4*)m + i),
              vv = __builtin_nontemporal_load((f32x4*)v + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pp[e], me = mm[e], ve = vv[e];
            adam_update<COEF, DECAY>(pe, gg[e], me, ve, dec, k);
            pp[e] = pe; mm[e] = me; vv[e] = ve;
        }
        ((f32x4*)p)[i] = pp; __builtin_nontemporal_store(mm, (f32x4*)m + i); __builtin_nontemporal_store(vv, (f32x4*)v + i);
    }
    // tail: at most three elements
    for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const bool dec = DECAY ? decay_bit(bits, first_block + (i >> 6)) : false;
        float pe = p[i], me = m[i], ve = v[i];
        adam_update<COEF, DECAY>(pe, g[i], me, ve, dec, k);
        m[i] = me; v[i] = ve; p[i] = pe;
    }
}

// Step counter kept on the device (so that a captured hipGraph can be replayed): state[0] = step count t (as float bits of an int),
// state[1] = lr f / (1 - b1^t), state[2] = 1 / sqrt(1 - b2^t) and, with write_decay, state[3] = 1 - lr f wd, f = factor(step_offset + t - 1).
// cpc_adam_dev is the constant schedule (f is exactly 1.0) without write_decay: state[3] stays as the caller left it.
__global__ void adam_tick_kernel(float* __restrict__ state, float lr, float b1, float b2, float weight_decay, int write_decay, int kind,
                                 long long warmup, long long total, float min_ratio, long long step_offset,
                                 const float* __restrict__ skip) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (skip && skip[0] != 0.f) return;
    int t = __float_as_int(state[0]) + 1;
    state[0] = __int_as_float(t);
    const double lrs = (double)lr * lr_factor(kind, warmup, total, (double)min_ratio, step_offset + t - 1);
    const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
    state[1] = (float)(lrs / bc1);
    state[2] = (float)(1.0 / sqrt(bc2));
    if (write_decay) state[3] = (float)(1.0 - lrs * (double)weight_decay);
}

template <bool COEF, bool DECAY>
static void adam_launch(const AdamArgs& a, float step_size, float inv_bc2_sqrt, float decay, const float* state, int blocks,
                        hipStream_t stream) {
    hipLaunchKernelGGL((adam_kernel<COEF, DECAY>), dim3(blocks), dim3(256), 0, stream, a.p, a.g, a.m, a.v, a.n, step_size, a.b1, a.b2, a.eps,
                       inv_bc2_sqrt, a.grad_scale, decay, state, a.coef, a.decay_bits, a.first_block, a.skip);
}

// The streaming launch of every entry point: COEF = a coefficient is given, DECAY = weight_decay > 0 (the bitmap is not read otherwise).
static int adam_stream(const AdamArgs& a, float step_size, float inv_bc2_sqrt, float decay, const float* state, hipStream_t stream) {
    const int blocks = (int)min((long long)2048, (a.n / 4 + 255) / 256 + 1);
    const bool decays = a.weight_decay > 0.f;
    (a.coef ? (decays ? adam_launch<true, true> : adam_launch<true, false>)
            : (decays ? adam_launch<false, true> : adam_launch<false, false>))(a, step_size, inv_bc2_sqrt, decay, state, blocks, stream);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// What every entry point refuses (include/cpc_hip.h); cpc_adam, cpc_adam_clip and cpc_adam_dev come with weight_decay 0 and first_block 0.
static bool adam_args_ok(const AdamArgs& a) {
    if (!a.p || !a.g || !a.m || !a.v || a.n <= 0 || a.first_block < 0) return false;
    if (!(a.weight_decay >= 0.f) || !(a.weight_decay <= 3.402823466e38f)) return false;          // negative, NaN or inf
    return !(a.weight_decay > 0.f && !a.decay_bits);
}

// Host-side step count: cpc_adam, cpc_adam_clip (clip: the coefficient is not optional) and cpc_adamw.
int launch_adam(const AdamArgs& a, int step, bool clip, hipStream_t stream) {
    if (!adam_args_ok(a) || step < 1 || (clip && !a.coef)) return CPC_EINVAL;
    const double bc1 = 1.0 - pow((double)a.b1, step), bc2 = 1.0 - pow((double)a.b2, step);
    return adam_stream(a, (float)((double)a.lr / bc1), (float)(1.0 / sqrt(bc2)), (float)(1.0 - (double)a.lr * (double)a.weight_decay),
                       nullptr, stream);
}

// Device-side step count: cpc_adam_dev (adamw false: the constant schedule, state[3] untouched) and cpc_adamw_dev.
int launch_adam_dev(const AdamArgs& a, float* state, bool adamw, int kind, long long warmup_steps, long long total_steps, float min_ratio,
                    long long step_offset, hipStream_t stream) {
    if (!adam_args_ok(a) || !state || a.coef || step_offset < 0 || !lr_schedule_ok(kind, warmup_steps, total_steps, min_ratio))
        return CPC_EINVAL;
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, stream, state, a.lr, a.b1, a.b2, a.weight_decay, adamw ? 1 : 0, kind,
                       warmup_steps, total_steps, min_ratio, step_offset, a.skip);
    return adam_stream(a, 0.f, 0.f, 1.f, state, stream);
}

// ---- LAMB layer-wise trust ratios (include/cpc_hip.h: cpc_lamb; DESIGN.md, "LAMB trust ratios") ----
// adam_update's moments, then per parameter tensor P:  u = r + wd p (selected) or r,  r = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps);
// trust = ||p|| / ||u|| where P is selected and both norms are finite and > 0, else 1;  p -= lr * trust * u.  Three launches over a
// range of whole parameters (n is a multiple of 64: a parameter's alignment padding is zero, gives u = 0 and stays zero):
//   1. lamb_moments_kernel: m, v, and the sums of p^2 and u^2 of every 64-float block (workspace[2 blk], [2 blk + 1], blk absolute);
//   2. lamb_ratio_kernel:   one workgroup per parameter adds its blocks' sums and writes trust[0..2][param];
//   3. lamb_apply_kernel:   u again from the stored m, v and the old p (lamb_direction, the text pass 1 runs), then p.
// Every sum has a fixed shape and there is no atomic: the same data give the same bits for any grid and any split into ranges.
// Roundings on the longest path from an element to a parameter's sum of squares (tests/test_lamb_gpu.py computes its bound from them):
//   4 (a lane's four squares: one product, three fmas) + 4 (xor-shuffle levels 8, 4, 2, 1 inside the block's 16 lanes)
//   + ceil(blocks / (256 LAMB_CHAINS)) (a thread's chain) + 2 (its LAMB_CHAINS = 4 chains) + 6 (wave tree) + 2 (four waves):
//   34 for the 16 384 blocks of the headline model's layer-2 kernel.
struct LambStep { float lr, inv_bc1, inv_bc2_sqrt, wd, b1, b2, eps, grad_scale, cf; };
constexpr int LAMB_CHAINS = 4;

// The moments of one element: adam_update's formulas with every fma written out and contraction off, so that the COEF and the plain
// instantiation round alike (left to itself the compiler pairs the second moment's products differently in the two, as it does for
// adam_kernel's scalar arguments); with cf == 1 and an exact g * grad_scale the two give the same bits.
template <bool COEF>
__device__ __forceinline__ void lamb_moments(float g, float& m, float& v, const LambStep& k) {
#pragma clang fp contract(off)
    float ge = g * k.grad_scale;
    if (COEF) ge = ge * k.cf;
    m = __builtin_fmaf(ge - m, 1.f - k.b1, m);
    v = __builtin_fmaf((1.f - k.b2) * ge, ge, v * k.b2);
}

// LAMB's direction of one element, the only copy of it: passes 1 and 3 run this text, with its one fma written out and
// contraction off, and so give the same bits.
__device__ __forceinline__ float lamb_direction(float p, float m, float v, bool sel, const LambStep& k) {
#pragma clang fp contract(off)
    const float r = (m * k.inv_bc1) / (sqrtf(v) * k.inv_bc2_sqrt + k.eps);
    return sel ? __builtin_fmaf(k.wd, p, r) : r;
}

template <bool COEF>
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long long n4, LambStep k,
                                                           const float* __restrict__ coef, const unsigned* __restrict__ bits,
                                                           long long first_block, float* __restrict__ ws,
                                                           const float* __restrict__ skip) {
    if (skip && skip[0] != 0.f) return;
    if (COEF) k.cf = coef[0];
    // n4 is a multiple of 16 and so is the grid's stride: the 16 lanes of a block enter and leave the loop together
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const long long blk = first_block + (i >> 4);
        const bool sel = decay_bit(bits, blk);
        const f32x4 pp = ((const f32x4*)p)[i], gg = __builtin_nontemporal_load((const f32x4*)g + i);
        f32x4 mm = __builtin_nontemporal_load((f32x4*)m + i), vv = __builtin_nontemporal_load((f32x4*)v + i);
        float sp = 0.f, su = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float me = mm[e], ve = vv[e];
            lamb_moments<COEF>(gg[e], me, ve, k);
            mm[e] = me; vv[e] = ve;
            const float u = lamb_direction(pp[e], me, ve, sel, k);
            sp = e ? __builtin_fmaf(pp[e], pp[e], sp) : pp[e] * pp[e];
            su = e ? __builtin_fmaf(u, u, su) : u * u;
        }
        // gradient and moments non-temporal, as in adam_kernel: they must not push the backward GEMMs' operands out of the cache
        __builtin_nontemporal_store(mm, (f32x4*)m + i); __builtin_nontemporal_store(vv, (f32x4*)v + i);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { sp += __shfl_xor(sp, o, 64); su += __shfl_xor(su, o, 64); }
        if ((threadIdx.x & 15) == 0) ((float2*)ws)[blk] = make_float2(sp, su);
    }
}

// One workgroup per parameter of the range: thread t adds the block sums t + 256 c into chain c % LAMB_CHAINS, in that order.
// trust[0][q] = ||p||, trust[1][q] = ||u||, trust[2][q] = the ratio pass 3 applies (rows of total_params floats).
__global__ __launch_bounds__(256) void lamb_ratio_kernel(const float* __restrict__ ws, const int* __restrict__ param_block,
                                                         int first_param, int total_params, const unsigned* __restrict__ bits,
                                                         float trust_clip, float* __restrict__ trust, const float* __restrict__ skip) {
    __shared__ float lds_p[4], lds_u[4];
    if (skip && skip[0] != 0.f) return;
    const int q = first_param + blockIdx.x;
    const int b0 = param_block[q], b1 = param_block[q + 1];
    float ap[LAMB_CHAINS] = {0.f, 0.f, 0.f, 0.f}, au[LAMB_CHAINS] = {0.f, 0.f, 0.f, 0.f};
    for (int j = b0 + (int)threadIdx.x; j < b1; j += 256 * LAMB_CHAINS) {
#pragma unroll
        for (int c = 0; c < LAMB_CHAINS; ++c)
            if (j + 256 * c < b1) {
                const float2 s = ((const float2*)ws)[j + 256 * c];
                ap[c] += s.x; au[c] += s.y;
            }
    }
    const float sp = gn_block_sum((ap[0] + ap[1]) + (ap[2] + ap[3]), lds_p);
    const float su = gn_block_sum((au[0] + au[1]) + (au[2] + au[3]), lds_u);
    if (threadIdx.x != 0) return;
    const float w_norm = sqrtf(sp), u_norm = sqrtf(su);
    const bool usable = w_norm > 0.f && u_norm > 0.f && w_norm <= 3.402823466e38f && u_norm <= 3.402823466e38f;          // finite, not NaN
    float ratio = (decay_bit(bits, b0) && usable) ? w_norm / u_norm : 1.f;
    if (trust_clip > 0.f) ratio = fminf(ratio, trust_clip);
    trust[q] = w_norm;
    trust[total_params + q] = u_norm;
    trust[2 * (long long)total_params + q] = ratio;
}

// block_param[blk] = the parameter block blk belongs to: a 4-byte load the block's 16 lanes share, from a map that stays in cache
// (463 KB at 7.4 M parameters), against a search of the table per float4.
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                         long long n4, LambStep k, const unsigned* __restrict__ bits,
                                                         long long first_block, const int* __restrict__ block_param,
                                                         const float* __restrict__ ratio, const float* __restrict__ skip) {
    if (skip && skip[0] != 0.f) return;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const long long blk = first_block + (i >> 4);
        const bool sel = decay_bit(bits, blk);
        const float step = k.lr * ratio[block_param[blk]];
        f32x4 pp = ((f32x4*)p)[i];
        const f32x4 mm = __builtin_nontemporal_load((const f32x4*)m + i), vv = __builtin_nontemporal_load((const f32x4*)v + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) pp[e] = pp[e] - step * lamb_direction(pp[e], mm[e], vv[e], sel, k);
        ((f32x4*)p)[i] = pp;
    }
}

long long lamb_workspace_floats(long long total_blocks) { return total_blocks > 0 ? 2 * total_blocks : 0; }

int launch_lamb(const AdamArgs& a, int step, const LambTables& t, hipStream_t stream) {
    if (!adam_args_ok(a) || step < 1 || !a.decay_bits) return CPC_EINVAL;
    if (!t.param_block || !t.param_block_dev || !t.block_param || !t.workspace || !t.trust) return CPC_EINVAL;
    if ((uintptr_t)t.workspace % 8) return CPC_EINVAL;          // a block's two sums travel as one 8-byte store and load
    if (t.n_params <= 0 || t.first_param < 0 || t.total_params <= 0 || (long long)t.first_param + t.n_params > t.total_params)
        return CPC_EINVAL;
    if (!(t.trust_clip < 0.f) && !(t.trust_clip > 0.f && t.trust_clip <= 3.402823466e38f)) return CPC_EINVAL;
    // the range is whole parameters: the host's copy of the table has to give it the blocks the caller says it has
    const int* tb = t.param_block + t.first_param;
    for (int q = 0; q < t.n_params; ++q)
        if (tb[q + 1] < tb[q]) return CPC_EINVAL;
    if (tb[0] != a.first_block || 64LL * ((long long)tb[t.n_params] - tb[0]) != a.n) return CPC_EINVAL;
    const double bc1 = 1.0 - pow((double)a.b1, step), bc2 = 1.0 - pow((double)a.b2, step);
    const LambStep k = {a.lr, (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)), a.weight_decay, a.b1, a.b2, a.eps, a.grad_scale, 1.f};
    const long long n4 = a.n / 4;
    const int blocks = (int)min((long long)2048, (n4 + 255) / 256);
    if (a.coef)
        hipLaunchKernelGGL(lamb_moments_kernel<true>, dim3(blocks), dim3(256), 0, stream, (const float*)a.p, a.g, a.m, a.v, n4, k, a.coef,
                           a.decay_bits, a.first_block, t.workspace, a.skip);
    else
        hipLaunchKernelGGL(lamb_moments_kernel<false>, dim3(blocks), dim3(256), 0, stream, (const float*)a.p, a.g, a.m, a.v, n4, k, a.coef,
                           a.decay_bits, a.first_block, t.workspace, a.skip);
    hipLaunchKernelGGL(lamb_ratio_kernel, dim3(t.n_params), dim3(256), 0, stream, (const float*)t.workspace, t.param_block_dev,
                       t.first_param, t.total_params, a.decay_bits, t.trust_clip, t.trust, a.skip);
    hipLaunchKernelGGL(lamb_apply_kernel, dim3(blocks), dim3(256), 0, stream, a.p, (const float*)a.m, (const float*)a.v, n4, k,
                       a.decay_bits, a.first_block, t.block_param, (const float*)(t.trust + 2LL * t.total_params), a.skip);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// ---- EMA of the weights (include/cpc_hip.h: cpc_ema, cpc_ema_swap; DESIGN.md, "EMA of the weights") ----
// ema = ema + (p - ema) * w, w = 1 - d: the difference rounds once and the product and the sum are one fma written out, so that the
// float4 body and the tail run the same arithmetic and a buffer averaged in pieces carries the whole call's bits.  w == 1 (decay 0) is
// the exact result p: (p - ema) + ema rounds twice and would not give it.
__device__ __forceinline__ float ema_update(float e, float p, float w) {
#pragma clang fp contract(off)
    return w == 1.f ? p : __builtin_fmaf(p - e, w, e);
}

// A launch of its own behind the update (adam_kernel's text is pinned by its tests' bits), of adam_kernel's shape.  With ``state``
// (FusedAdam.state, advanced by adam_tick_kernel in front of the update) every thread derives w from the device's step count t:
// 1 - min(decay, (1 + t) / (10 + t)) = max(1 - decay, 9 / (10 + t)), one correctly rounded float division where the host divides in
// double and rounds once — at most one unit in the last place of w apart.  Otherwise w is the argument.
__global__ __launch_bounds__(256) void ema_kernel(const float* __restrict__ p, float* __restrict__ ema, long long n, float w, float decay,
                                                  int warmup, const float* __restrict__ state, const float* __restrict__ skip) {
    // NaN guard, as in adam_kernel: the update in front of this launch was a no-op, so the average stays where it is too
    if (skip && skip[0] != 0.f) return;
    if (state) {
        w = 1.f - decay;
        if (warmup) w = fmaxf(w, 9.f / (10.f + (float)__float_as_int(state[0])));
    }
    const long long n4 = n / 4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        // the parameters were just written and are read again by the layout kernels: a plain load.  The average is touched once per
        // step: non-temporal both ways, as adam_kernel's moments, so that it does not push the backward GEMMs' operands out of the cache
        const f32x4 pp = ((const f32x4*)p)[i];
        f32x4 ee = __builtin_nontemporal_load((f32x4*)ema + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) ee[e] = ema_update(ee[e], pp[e], w);
        __builtin_nontemporal_store(ee, (f32x4*)ema + i);
    }
    // tail: at most three elements
    for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) ema[i] = ema_update(ema[i], p[i], w);
}

__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema, long long n) {
    const long long n4 = n / 4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const f32x4 pp = ((const f32x4*)p)[i], ee = __builtin_nontemporal_load((const f32x4*)ema + i);
        ((f32x4*)p)[i] = ee;
        __builtin_nontemporal_store(pp, (f32x4*)ema + i);
    }
    for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float pe = p[i];
        p[i] = ema[i];
        ema[i] = pe;
    }
}

// What both entry points refuse: the buffers move as float4.
static bool ema_args_ok(const float* p, const float* ema, long long n) {
    return p && ema && n > 0 && !((uintptr_t)p % 16) && !((uintptr_t)ema % 16);
}

// adam_stream's grid: at most 2048 workgroups walk the float4 bodies with a grid stride, the "+ 1" keeps a thread for the tail.
static int ema_blocks(long long n) { return (int)min((long long)2048, (n / 4 + 255) / 256 + 1); }

int launch_ema(const float* p, float* ema, long long n, float decay, int warmup, int step, const float* state, const float* skip,
               hipStream_t stream) {
    if (!ema_args_ok(p, ema, n) || !(decay >= 0.f && decay < 1.f) || (!state && step < 1)) return CPC_EINVAL;          // NaN fails the range
    float w = 0.f;
    if (!state) {          // in double, rounded once
        double d = (double)decay;
        if (warmup) d = fmin(d, (1.0 + (double)step) / (10.0 + (double)step));
        w = (float)(1.0 - d);
    }
    hipLaunchKernelGGL(ema_kernel, dim3(ema_blocks(n)), dim3(256), 0, stream, p, ema, n, w, decay, warmup ? 1 : 0, state, skip);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_ema_swap(float* p, float* ema, long long n, hipStream_t stream) {
    if (!ema_args_ok(p, ema, n)) return CPC_EINVAL;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(ema_blocks(n)), dim3(256), 0, stream, p, ema, n);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// Operands of a tall (kh,1) convolution computed G output rows per GEMM row (scalogram_engine._col_group): G shifted copies of the kernel
// in a window of Rw (forward) / Rd (data gradient) rows, zero elsewhere.  W f32 [co][c][kh];
//   fwd  [dh][co][r][c]  = W[co][c][r - dh]              for dh <= r < dh + kh      (output row G R + dh reads window rows dh .. dh+kh-1)
//   dgrd [dr][c][q][co]  = W[co][c][kh - 1 - (q - dr)]   for dr <= q < dr + kh      (input row G R + dr receives tap j from dY window row dr + kh-1 - j)
//   bias_g [dh][co] = bias[co]   (bias may be null)
// One thread per output element, the fastest index of each layout along the lanes (the weights are a few MB; this replaces 3 G small
// copy / flip launches per convolution and step).
template <typename T>
__global__ __launch_bounds__(256) void conv_w_prep_group_kernel(const float* __restrict__ W, const float* __restrict__ bias,
                                                                T* __restrict__ fwd, T* __restrict__ dgrd, float* __restrict__ bias_g,
                                                                int Cout, int Cin, int kh, int G, int Rw, int Rd) {
    const long long nf = (long long)G * Cout * Rw * Cin, nd = (long long)G * Cin * Rd * Cout;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nf) {
        const int c = (int)(i % Cin), r = (int)((i / Cin) % Rw), co = (int)((i / ((long long)Cin * Rw)) % Cout), dh = (int)(i / ((long long)Cin * Rw * Cout));
        const int j = r - dh;
        fwd[i] = from_f32<T>((j >= 0 && j < kh) ? W[((long long)co * Cin + c) * kh + j] : 0.f);
    } else if (i < nf + nd) {
        const long long k = i - nf;
        const int co = (int)(k % Cout), q = (int)((k / Cout) % Rd), c = (int)((k / ((long long)Cout * Rd)) % Cin), dr = (int)(k / ((long long)Cout * Rd * Cin));
        const int j = kh - 1 - (q - dr);
        dgrd[k] = from_f32<T>((j >= 0 && j < kh) ? W[((long long)co * Cin + c) * kh + j] : 0.f);
    } else if (bias && i < nf + nd + (long long)G * Cout) {
        const long long k = i - nf - nd;
        bias_g[k] = bias[k % Cout];
    }
}

int launch_conv_w_prep_group(const float* W, const float* bias, void* fwd, void* dgrd, float* bias_g, int Cout, int Cin, int kh, int G,
                             int Rw, int Rd, int dtype, hipStream_t stream) {
    if (Cout <= 0 || Cin <= 0 || kh <= 0 || G <= 0 || Rw < kh + G - 1 || Rd < kh + G - 1 || !W || !fwd || !dgrd || (bias && !bias_g))
        return CPC_EINVAL;
    const long long n = (long long)G * Cout * Rw * Cin + (long long)G * Cin * Rd * Cout + (long long)G * Cout;
    const long long blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return CPC_EINVAL;
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((conv_w_prep_group_kernel<bf16_t>), dim3((unsigned)blocks), dim3(256), 0, stream, W, bias, (bf16_t*)fwd, (bf16_t*)dgrd,
                           bias_g, Cout, Cin, kh, G, Rw, Rd);
    else if (dtype == CPC_DTYPE_F32)
        hipLaunchKernelGGL((conv_w_prep_group_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, stream, W, bias, (float*)fwd, (float*)dgrd,
                           bias_g, Cout, Cin, kh, G, Rw, Rd);
    else
        return CPC_EINVAL;
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// Host side of the batched form: fills the launch geometry of every job (D, tco, gx, first workgroup) and returns the grid size and the
// dynamic LDS the launch needs; the caller uploads the table once (operand addresses are stable) and launches with those.
int conv_w_prep_plan(void* jobs_host, int njobs, int* total_blocks, int* lds_bytes) {
    if (!jobs_host || njobs <= 0 || njobs > 4096 || !total_blocks || !lds_bytes) return CPC_EINVAL;
    ConvPrepJob* jobs = (ConvPrepJob*)jobs_host;
    long long first = 0;
    size_t lds = 0;
    for (int j = 0; j < njobs; ++j) {
        ConvPrepJob& q = jobs[j];
        if (q.Cout <= 0 || q.Cin <= 0 || q.kw <= 0 || q.stride <= 0 || q.kw > 511 || !q.W || (!q.fwd && !q.dgrd)) return CPC_EINVAL;
        q.D = (q.kw + q.stride - 1) / q.stride;
        int tco = 32;
        while (tco > 1 && (long long)tco * (32 * q.kw + 1) > 16384) tco >>= 1;
        q.tco = tco;
        q.gx = (q.Cin + 31) / 32;
        q.first = (int)first;
        first += (long long)q.gx * ((q.Cout + tco - 1) / tco);
        if (first > 0x7fffffffLL) return CPC_EINVAL;
        lds = std::max(lds, (size_t)tco * (32 * q.kw + 1) * sizeof(float));
    }
    *total_blocks = (int)first;
    *lds_bytes = (int)lds;
    return CPC_OK;
}

int launch_conv_w_prep_batch(const void* jobs_dev, int njobs, int total_blocks, int lds_bytes, int dtype, hipStream_t stream) {
    if (!jobs_dev || njobs <= 0 || total_blocks <= 0 || lds_bytes <= 0 || lds_bytes > 65536) return CPC_EINVAL;
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((conv_w_prep_batch_kernel<bf16_t>), dim3(total_blocks), dim3(256), (size_t)lds_bytes, stream, (const ConvPrepJob*)jobs_dev, njobs);
    else if (dtype == CPC_DTYPE_F32)
        hipLaunchKernelGGL((conv_w_prep_batch_kernel<float>), dim3(total_blocks), dim3(256), (size_t)lds_bytes, stream, (const ConvPrepJob*)jobs_dev, njobs);
    else
        return CPC_EINVAL;
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_conv_w_prep(const float* W, void* fwd, void* dgrd, int Cout, int Cin, int kw, int stride, int dtype,
                       hipStream_t stream) {
    if (Cout <= 0 || Cin <= 0 || kw <= 0 || stride <= 0) return CPC_EINVAL;
    const int D = (kw + stride - 1) / stride;
    if (kw > 511) return CPC_EINVAL;
    int tco = 32;                                                            // LDS tile of at most 64 KiB: fewer co for very wide kernels
    while (tco > 1 && (long long)tco * (32 * kw + 1) > 16384) tco >>= 1;
    // (a 512 x 512 x 8 weight is 256 tiles of 32 x 32 channels: one workgroup per CU, each walking 96 elements per thread through index
    // arithmetic with nothing to hide its latency behind — 65 us for 2 M elements; 4 output channels per tile, eight times the workgroups: 25 us; 45 / 31 / 27 / 25 / 25 us at 32 / 16 / 8 / 4 / 2)
    while (tco > 4 && (long long)((Cin + 31) / 32) * ((Cout + tco - 1) / tco) < 2048) tco >>= 1;
    const dim3 grid((Cin + 31) / 32, (Cout + tco - 1) / tco);
    const size_t lds = (size_t)tco * (32 * kw + 1) * sizeof(float);
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((conv_w_prep_kernel<bf16_t>), grid, dim3(256), lds, stream, W, (bf16_t*)fwd, (bf16_t*)dgrd, Cout,
                           Cin, kw, stride, D, tco);
    else if (dtype == CPC_DTYPE_F32)
        hipLaunchKernelGGL((conv_w_prep_kernel<float>), grid, dim3(256), lds, stream, W, (float*)fwd, (float*)dgrd, Cout, Cin,
                           kw, stride, D, tco);
    else
        return CPC_EINVAL;
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_cast2d(const float* src, void* dst, int R, int C, long long sr, long long sc, int dtype, hipStream_t stream) {
    if (R <= 0 || C <= 0) return CPC_EINVAL;
    const long long n = (long long)R * C;
    const int blocks = (int)min((long long)2048, (n + 255) / 256);
    if (n >= 4096 && (C + 31) / 32 <= 65535 && (R + 31) / 32 <= 65535) {
        const dim3 grid((C + 31) / 32, (R + 31) / 32);
        if (dtype == CPC_DTYPE_BF16)
            hipLaunchKernelGGL((cast2d_tile_kernel<bf16_t>), grid, dim3(256), 0, stream, src, (bf16_t*)dst, R, C, sr, sc);
        else if (dtype == CPC_DTYPE_F32)
            hipLaunchKernelGGL((cast2d_tile_kernel<float>), grid, dim3(256), 0, stream, src, (float*)dst, R, C, sr, sc);
        else
            return CPC_EINVAL;
        CPC_CHECK_LAUNCH();
        return CPC_OK;
    }
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((cast2d_kernel<bf16_t>), dim3(blocks), dim3(256), 0, stream, src, (bf16_t*)dst, R, C, sr, sc);
    else if (dtype == CPC_DTYPE_F32)
        hipLaunchKernelGGL((cast2d_kernel<float>), dim3(blocks), dim3(256), 0, stream, src, (float*)dst, R, C, sr, sc);
    else
        return CPC_EINVAL;
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_cast2d_batch(const void* jobs, int njobs, int dtype, hipStream_t stream) {
    if (!jobs || njobs <= 0 || njobs > 65535) return CPC_EINVAL;
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((cast2d_batch_kernel<bf16_t>), dim3(64, njobs), dim3(256), 0, stream, (const CastJob*)jobs);
    else if (dtype == CPC_DTYPE_F32)
        hipLaunchKernelGGL((cast2d_batch_kernel<float>), dim3(64, njobs), dim3(256), 0, stream, (const CastJob*)jobs);
    else
        return CPC_EINVAL;
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_maxpool_fwd(const void* in, void* out, int B, int C, int pool, int Lin_valid, int Lin_alloc, int Lout_valid,
                       int Lout_alloc, int dtype, hipStream_t stream) {
    if (B <= 0 || C <= 0 || C % 4 || pool < 1 || Lin_valid <= 0 || Lin_alloc < Lin_valid || Lout_valid <= 0 || Lout_alloc < Lout_valid ||
        (long long)(Lout_valid - 1) * pool >= Lin_valid)
        return CPC_EINVAL;
    const long long total = (long long)B * Lout_alloc * (C / 4);
    const int blocks = (int)min((long long)2048, (total + 255) / 256);
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((maxpool_fwd_kernel<bf16_t>), dim3(blocks), dim3(256), 0, stream, (const bf16_t*)in, (bf16_t*)out, B, C, pool,
                           Lin_valid, Lin_alloc, Lout_valid, Lout_alloc);
    else if (dtype == CPC_DTYPE_F32)
        hipLaunchKernelGGL((maxpool_fwd_kernel<float>), dim3(blocks), dim3(256), 0, stream, (const float*)in, (float*)out, B, C, pool,
                           Lin_valid, Lin_alloc, Lout_valid, Lout_alloc);
    else
        return CPC_EINVAL;
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_maxpool_bwd(const void* in, const void* dout, void* din, int B, int C, int pool, int Lin_valid, int Lin_alloc,
                       int Lout_alloc, int dtype, hipStream_t stream) {
    if (B <= 0 || C <= 0 || C % 4 || pool < 1 || Lin_valid <= 0 || Lin_alloc < Lin_valid || Lout_alloc <= 0 ||
        (Lin_valid - 1) / pool >= Lout_alloc)
        return CPC_EINVAL;
    const long long total = (long long)B * Lin_alloc * (C / 4);
    const int blocks = (int)min((long long)2048, (total + 255) / 256);
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((maxpool_bwd_kernel<bf16_t>), dim3(blocks), dim3(256), 0, stream, (const bf16_t*)in, (const bf16_t*)dout,
                           (bf16_t*)din, B, C, pool, Lin_valid, Lin_alloc, Lout_alloc);
    else if (dtype == CPC_DTYPE_F32)
        hipLaunchKernelGGL((maxpool_bwd_kernel<float>), dim3(blocks), dim3(256), 0, stream, (const float*)in, (const float*)dout,
                           (float*)din, B, C, pool, Lin_valid, Lin_alloc, Lout_alloc);
    else
        return CPC_EINVAL;
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_relu_row_bwd(const float* dc, const void* y, void* dy, int B, int C, long long item_stride, long long row_off, int dtype,
                        hipStream_t stream) {
    if (B <= 0 || C <= 0) return CPC_EINVAL;
    const int blocks = min(1024, (B * C + 255) / 256);
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((relu_row_bwd_kernel<bf16_t>), dim3(blocks), dim3(256), 0, stream, dc, (const bf16_t*)y, (bf16_t*)dy, B, C,
                           item_stride, row_off);
    else if (dtype == CPC_DTYPE_F32)
        hipLaunchKernelGGL((relu_row_bwd_kernel<float>), dim3(blocks), dim3(256), 0, stream, dc, (const float*)y, (float*)dy, B, C,
                           item_stride, row_off);
    else
        return CPC_EINVAL;
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// ---- sign-bit masks (include/cpc_hip.h, cpc_sign_bits): out[i] bit e = x[8 i + e] > 0.  A block turns 8192 elements into 1 KiB:
// four passes in which thread t takes the 8 elements 2048 q + 8 t (16-byte loads, contiguous over the wave) and writes byte 256 q + t.
template <typename T>
__global__ __launch_bounds__(256) void sign_bits_kernel(const T* __restrict__ x, unsigned char* __restrict__ out, long long n8) {
    const long long nchunk = (n8 + 1023) / 1024;
    for (long long c = blockIdx.x; c < nchunk; c += gridDim.x) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long i = c * 1024 + q * 256 + threadIdx.x;          // 8-element group
            if (i >= n8) break;
            unsigned b8 = 0;
            if constexpr (sizeof(T) == 2) {
                const uint4 v = *(const uint4*)(x + i * 8);
                const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // bf16 > 0  <=>  not zero and sign clear  <=>  (h - 1) < 0x7fff
                    b8 |= (((w4[e] & 0xffffu) - 1u) < 0x7fffu ? 1u : 0u) << (2 * e);
                    b8 |= (((w4[e] >> 16) - 1u) < 0x7fffu ? 1u : 0u) << (2 * e + 1);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) b8 |= ((float)x[i * 8 + e] > 0.f ? 1u : 0u) << e;
            }
            out[i] = (unsigned char)b8;
        }
    }
}

int launch_sign_bits(const void* x, unsigned char* bits, long long n, int dtype, hipStream_t stream) {
    if (n % 32 || ((uintptr_t)x % 16) || ((uintptr_t)bits % 4)) return CPC_EINVAL;
    const long long n8 = n / 8;
    const unsigned grid = (unsigned)std::min<long long>((n8 + 1023) / 1024, 256 * 32);
    if (dtype == CPC_DTYPE_BF16) hipLaunchKernelGGL(sign_bits_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)x, bits, n8);
    else if (dtype == CPC_DTYPE_F32) hipLaunchKernelGGL(sign_bits_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)x, bits, n8);
    else return CPC_EINVAL;
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// ------------------------------------------------------------------------------------------- prediction anchors: target gradients
// cpc_anchor_target_grad: the top-layer gradient rows that the target windows of A anchors share.  dT f32 [A][B][K][E] holds every
// anchor's d loss / d targets; the window of anchor a covers top rows [first_row + a stride, first_row + a stride + K).  A gather per
// output row: a thread owns one 16-byte piece (CH channels) of one row r in [row_lo, row_hi) of one item and sums, in f32 and with a
// ascending, the pieces dT[a][b][r - first_row - a stride] of the windows that cover r — the anchors a in [a_lo, a_hi], worked out
// from the arguments alone, so the order of the sum is fixed and nothing is atomic.  ACC adds the stored row first-to-last behind the
// sum (one rounding); a row no window covers is written as zeros (ACC == 0) or not touched (ACC).  Channels on the lanes: a wave reads
// 64 consecutive 16- or 32-byte pieces of a dT row per anchor and writes 1 KiB of the output row.
template <typename T, bool ACC>
__global__ __launch_bounds__(256) void anchor_target_grad_kernel(const float* __restrict__ dT, T* __restrict__ dtop, long long item,
                                                                 int A, int B, int K, int E, long long first_row, long long stride,
                                                                 int row_lo, int nrows) {
    constexpr int CH = Elem<T>::CH;
    const int pieces = E / CH;
    const long long total = (long long)B * nrows * pieces;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int p = (int)(i % pieces);
        const long long br = i / pieces;
        const int r = row_lo + (int)(br % nrows);
        const int b = (int)(br / nrows);
        // anchors with 0 <= r - first_row - a stride < K
        const long long rel = (long long)r - first_row;
        long long a_hi = rel >= 0 ? rel / stride : -1;
        const long long need = rel - (K - 1);                       // a stride >= need
        long long a_lo = need <= 0 ? 0 : (need + stride - 1) / stride;
        if (a_hi > A - 1) a_hi = A - 1;
        T* out = dtop + (long long)b * item + (long long)r * E + p * CH;
        if (a_lo > a_hi) {
            if constexpr (!ACC) {
                if constexpr (CH == 8) *(uint4*)out = make_uint4(0u, 0u, 0u, 0u);
                else *(f32x4*)out = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            continue;
        }
        float acc[CH];
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] = 0.f;
        for (long long a = a_lo; a <= a_hi; ++a) {
            const long long k = rel - a * stride;
            const float* src = dT + (((long long)a * B + b) * K + k) * E + p * CH;
#pragma unroll
            for (int q = 0; q < CH / 4; ++q) {
                const f32x4 v = *(const f32x4*)(src + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * q + e] += v[e];
            }
        }
        if constexpr (CH == 8) {
            bf16x8 o;
            if constexpr (ACC) {
                const bf16x8 old = *(const bf16x8*)out;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += (float)old[e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16_t)acc[e];
            *(bf16x8*)out = o;
        } else {
            f32x4 o;
            if constexpr (ACC) {
                const f32x4 old = *(const f32x4*)out;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += old[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = acc[e];
            *(f32x4*)out = o;
        }
    }
}

int launch_anchor_target_grad(const float* dT, void* dtop, long long item, int A, int B, int K, int E, int first_row, int stride,
                              int row_lo, int row_hi, int accumulate, int dtype, hipStream_t stream) {
    if (dtype != CPC_DTYPE_BF16 && dtype != CPC_DTYPE_F32) return CPC_EINVAL;
    const int ch = dtype == CPC_DTYPE_BF16 ? 8 : 4;
    if (!dT || !dtop || A < 1 || B < 1 || K < 1 || stride < 1 || E < 1 || E % ch) return CPC_EINVAL;
    if (row_lo < 0 || row_hi <= row_lo || first_row < 0) return CPC_EINVAL;
    if (item % ch || item < (long long)row_hi * E) return CPC_EINVAL;          // 16-byte pieces; the items' row ranges do not overlap
    const int nrows = row_hi - row_lo;
    const long long total = (long long)B * nrows * (E / ch);
    const int blocks = (int)min((long long)2048, (total + 255) / 256);          // 256 CUs x 8 blocks; the rest by the grid stride
#define ATG(T, ACC) \
    hipLaunchKernelGGL((anchor_target_grad_kernel<T, ACC>), dim3(blocks), dim3(256), 0, stream, dT, (T*)dtop, item, A, B, K, E, \
                       (long long)first_row, (long long)stride, row_lo, nrows)
    if (dtype == CPC_DTYPE_BF16) { if (accumulate) ATG(bf16_t, true); else ATG(bf16_t, false); }
    else { if (accumulate) ATG(float, true); else ATG(float, false); }
#undef ATG
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
