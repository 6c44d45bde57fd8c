// InfoNCE loss of ContrastiveEstimationTrainer.train (default branch: same-step scores only), forward + analytic
// gradient with respect to the linear scores.
//
//   S[k][b][b'] = <predicted_z[b,k,:], targets[b',:,k]>      (computed by a batched gemm_nt, f32)
//   sp = softplus(S) (softplus score) or S (linear score)
//   loss = -mean_{b,k} sp[k][b][b] + mean_{k,b'} logsumexp_b sp[k][b][b'] + reg * mean_{b,b'} (mean_k sp[k][b][b'])^2
//   dL/dS = dsp * (softplus ? sigmoid(S) : 1),
//   dsp[k][b][b'] = (softmax_b(sp[k][:,b'])[b] - [b == b']) / (B K) + 2 reg / (B^2 K) * mean_k sp[k][b][b']
//
// The softmax runs over the PREDICTION axis b for every target b' (columns), as the reference does.
#include "cpc_common.h"
#include "cpc_kernels.h"

namespace {

constexpr int NCE_CW = 8;       // columns per workgroup of the equal-step loss's column pass (nce_col_mean_kernel)

__device__ __forceinline__ float score_tf(float x, int softplus) {
    if (!softplus) return x;
    return x > 20.f ? x : log1pf(expf(x));       // torch.nn.functional.softplus, beta = 1, threshold = 20
}
__device__ __forceinline__ float score_grad(float x, int softplus) {
    if (!softplus) return 1.f;
    return x > 20.f ? 1.f : 1.f / (1.f + expf(-x));
}

// The block reduction of this file: N values per thread of a 256-thread workgroup, the first NSUM of them summed and the rest
// maximised, through red[N][256].  A fixed tree, strides 128 down to 1, the lower index taking the upper: the result depends on the
// values alone, never on timing.  Called by all 256 threads; every thread may read the results red[i][0] afterwards, and has to pass
// a barrier of its own before it writes red again.
template <int N, int NSUM = N>
__device__ __forceinline__ void block_reduce(float (&red)[N][256], const float (&v)[N]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < N; ++i) red[i][t] = v[i];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                if (i < NSUM) red[i][t] += red[i][t + s];
                else red[i][t] = fmaxf(red[i][t], red[i][t + s]);
            }
        }
        __syncthreads();
    }
}

// logsumexp over b of every (k, b') column.  grid (ceil(B/32), K, nsplit); block 256 = 32 columns x 8 row lanes, each lane keeps
// an online (max, sum) over its rows of the split's row range, combined through LDS.  With nsplit == 1 it writes lse[k][b'] and
// one partial sum of lse per block; otherwise the per-split (max, sum) pairs go to pm / ps [split][k][b'] for nce_col_merge_kernel
// (the all-timesteps matrix has 3072 rows but only 96 column blocks: the rows must be split to fill the chip).
// (body with explicit block coordinates: nce_col_kernel calls it with its own, nce_col_mean_kernel with a slice of a 1-D grid)
template <int CW>
__device__ __forceinline__ void nce_col_body(const float* __restrict__ S, float* __restrict__ lse, float* __restrict__ partial, int B,
                                             int K, int ld, int softplus, int rows_per_split, float* __restrict__ pm,
                                             float* __restrict__ ps, int bx, int by, int bz, int nbx, int nbz) {
    // CW columns x RL row lanes per workgroup.  The softplus / exp arithmetic is what this path costs (some hundred instructions per
    // score): with 32 columns per workgroup the equal-step loss (K x B columns of B rows) ran on 96 workgroups, a lane walking 32
    // rows; 8 columns x 32 row lanes spread the same work over four times as many waves (nce_col_mean_kernel: 18.6 -> 13.3 us at
    // B = 256, K = 12; more loads in flight per lane had changed nothing: it is the arithmetic, not the latency).
    constexpr int RL = 256 / CW;
    __shared__ float smx[RL][CW], ssum[RL][CW];
    const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
    const int k = by, bp = bx * CW + tx;
    const int r0 = bz * rows_per_split, r1 = min(B, r0 + rows_per_split);
    float mx = -INFINITY, sum = 0.f;
    if (bp < B) {
        const float* col = S + (long long)k * B * ld + bp;
        // eight rows per trip: the loads are independent of the running (max, sum), so they are in flight together
        for (int base = r0 + ty; base < r1; base += 8 * RL) {
            float vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) vv[u] = (base + RL * u < r1) ? col[(long long)(base + RL * u) * ld] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (base + RL * u < r1) {
                    const float v = score_tf(vv[u], softplus);
                    if (v > mx) { sum = sum * expf(mx - v) + 1.f; mx = v; }
                    else sum += expf(v - mx);
                }
            }
        }
    }
    smx[ty][tx] = mx;
    ssum[ty][tx] = sum;
    __syncthreads();
    if (ty == 0) {
        float m = mx;
#pragma unroll
        for (int r = 1; r < RL; ++r) m = fmaxf(m, smx[r][tx]);
        float tot = 0.f;
#pragma unroll
        for (int r = 0; r < RL; ++r)          // (a part whose max IS the column's max counts as it stands: with m = +inf, inf - inf would be NaN)
            tot += (smx[r][tx] == -INFINITY) ? 0.f : (smx[r][tx] == m) ? ssum[r][tx] : ssum[r][tx] * expf(smx[r][tx] - m);
        if (nbz > 1) {
            if (bp < B) {
                pm[((long long)bz * K + k) * B + bp] = m;
                ps[((long long)bz * K + k) * B + bp] = tot;
            }
            return;
        }
        const float l = (bp < B) ? m + logf(tot) : 0.f;
        if (bp < B) lse[k * B + bp] = l;
        // sum the CW columns of this block: shuffle reduction over the first CW lanes
        float acc = l;
        for (int o = CW / 2; o > 0; o >>= 1) acc += __shfl_down(acc, o, CW);
        if (tx == 0) partial[by * nbx + bx] = acc;
    }
}

__global__ __launch_bounds__(256) void nce_col_kernel(const float* __restrict__ S, float* __restrict__ lse,
                                                      float* __restrict__ partial, int B, int K, int ld, int softplus,
                                                      int rows_per_split, float* __restrict__ pm, float* __restrict__ ps) {
    nce_col_body<32>(S, lse, partial, B, K, ld, softplus, rows_per_split, pm, ps, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.z);
}

// Merges the per-split (max, sum) pairs of a column in split order: lse[c] and one partial sum of lse per block of 256 columns.
__global__ __launch_bounds__(256) void nce_col_merge_kernel(const float* __restrict__ pm, const float* __restrict__ ps, int nsplit,
                                                            int ncols, float* __restrict__ lse, float* __restrict__ partial) {
    __shared__ float red[1][256];
    const int c = blockIdx.x * 256 + threadIdx.x;
    float l = 0.f;
    if (c < ncols) {
        float m = -INFINITY;
        for (int z = 0; z < nsplit; ++z) m = fmaxf(m, pm[(long long)z * ncols + c]);
        float tot = 0.f;
        for (int z = 0; z < nsplit; ++z) {
            const float mz = pm[(long long)z * ncols + c];
            const float sz = ps[(long long)z * ncols + c];
            tot += (mz == -INFINITY) ? 0.f : (mz == m) ? sz : sz * expf(mz - m);          // (mz == m: as in nce_col_body)
        }
        l = m + logf(tot);
        lse[c] = l;
    }
    block_reduce<1>(red, {l});
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0][0];
}

// m[b][b'] = mean_k sp[k][b][b'] (the regulariser's mean over the prediction steps, contrastive_estimation_training.py:141)
// for every pair once, plus per-block partials {sum of the valid scores sp[k][b][b], sum m^2, max sp}.  (The gradient kernel
// used to recompute this mean in each of its K blocks per tile: 12 x the softplus work, 42 of the loss's 65 us.)
// ks: floats between the blocks of two steps k (B ld; the banked loss reads one slot of [K][slots B][ld]).
template <int KT>
__device__ __forceinline__ void nce_mean_body(const float* __restrict__ S, float* __restrict__ mean, float* __restrict__ partial, int B,
                                              int K_rt, int ld, int softplus, int bx, long long ks) {
    __shared__ float red[3][256];
    const int K = KT > 0 ? KT : K_rt;
    const long long idx = (long long)bx * 256 + threadIdx.x;
    float valid = 0.f, msq = 0.f, mx = -INFINITY;
    if (idx < (long long)B * B) {
        const int b = (int)(idx / B), bp = (int)(idx % B);
        const float* sp0 = S + (long long)b * ld + bp;
        float m = 0.f;
        if (KT > 0) {
            float raw[KT > 0 ? KT : 1];
#pragma unroll
            for (int k = 0; k < KT; ++k) raw[k] = sp0[k * ks];
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const float sp = score_tf(raw[k], softplus);
                m += sp;
                mx = fmaxf(mx, sp);
                if (b == bp) valid += sp;
            }
        } else {
            for (int k = 0; k < K; ++k) {
                const float sp = score_tf(sp0[k * ks], softplus);
                m += sp;
                mx = fmaxf(mx, sp);
                if (b == bp) valid += sp;
            }
        }
        m /= (float)K;
        msq = m * m;
        mean[(long long)b * ld + bp] = m;
    }
    block_reduce<3, 2>(red, {valid, msq, mx});
    if (threadIdx.x == 0) {
        partial[bx * 3 + 0] = red[0][0];
        partial[bx * 3 + 1] = red[1][0];
        partial[bx * 3 + 2] = red[2][0];
    }
}

// The column log-sum-exps and the pair means read the same scores and do not depend on each other: ONE launch, the first
// ncb * K workgroups take the columns, the rest the pairs (each launch of this latency-bound path costs 5-9 us by itself).
template <int KT>
__global__ __launch_bounds__(256) void nce_col_mean_kernel(const float* __restrict__ S, float* __restrict__ lse, float* __restrict__ colp,
                                                           float* __restrict__ mean, float* __restrict__ pairp, int B, int K, int ld,
                                                           int softplus, int ncb) {
    const int ncol = ncb * K;
    if ((int)blockIdx.x < ncol)
        nce_col_body<NCE_CW>(S, lse, colp, B, K, ld, softplus, B, nullptr, nullptr, blockIdx.x % ncb, blockIdx.x / ncb, 0, ncb, 1);
    else
        nce_mean_body<KT>(S, mean, pairp, B, K, ld, softplus, blockIdx.x - ncol, (long long)B * ld);
}

// out[0] = loss, out[1] = max score, out[2] = -mean valid, out[3] = mean lse, out[4] = reg term (already scaled)
__device__ __forceinline__ void nce_finalize_body(const float* __restrict__ col_partial, int ncol, const float* __restrict__ grad_partial,
                                                  int ngrad, float* __restrict__ out, int B, int K, float reg) {
    // fixed-shape tree reduction: the summation order depends only on (ncol, ngrad), not on timing
    __shared__ float red[4][256];
    float lse_sum = 0.f, valid = 0.f, msq = 0.f, mx = -INFINITY;
    for (int i = threadIdx.x; i < ncol; i += 256) lse_sum += col_partial[i];
    for (int i = threadIdx.x; i < ngrad; i += 256) {
        valid += grad_partial[i * 3 + 0];
        msq += grad_partial[i * 3 + 1];
        mx = fmaxf(mx, grad_partial[i * 3 + 2]);
    }
    block_reduce<4, 3>(red, {lse_sum, valid, msq, mx});
    if (threadIdx.x != 0) return;
    lse_sum = red[0][0]; valid = red[1][0]; msq = red[2][0]; mx = red[3][0];
    const float bk = (float)B * (float)K;
    const float t_valid = -valid / bk, t_lse = lse_sum / bk, t_reg = reg * msq / ((float)B * (float)B);
    out[0] = t_valid + t_lse + t_reg;
    out[1] = mx;
    out[2] = t_valid;
    out[3] = t_lse;
    out[4] = t_reg;
    // NaN guard of the reference (contrastive_estimation_training.py:124-133: isnan of the loss BEFORE the regulariser, then
    // `return` before backward() / optimizer.step()): out[5] = this step's indicator, out[6] = sticky (stays raised until the host
    // clears it) — cpc_adam / cpc_adam_dev skip their update while it is raised
    const float lb = t_valid + t_lse;
    const float bad = (lb != lb) ? 1.f : 0.f;
    out[5] = bad;
    if (bad != 0.f) out[6] = 1.f;
}

// ---- the gradient tile of the equal-step losses (dense, sampled / grouped, banked) ----
// What tells these losses apart is a column's candidate set, i.e. the coefficient dsp = d loss / d sp of one (b, b') pair.  A policy
// P says that much and nce_grad_tile does the rest:
//   P::column(k, bp)       once per thread before its rows (bp may lie past B): what the pairs of column (k, b') share
//   P::dsp(k, b, bp, sp)   the coefficient of a pair b, bp < B with transformed score sp
//   P::live, P::own        workgroup-uniform: the tile's rows have coefficients at all / are rows of the current batch
// The terms every policy puts its coefficient together from:
struct NceTerms {
    const float* lse;           // [K][B] column log-sum-exps over the candidates
    const float* mean;          // [B][ld] pair means (nce_mean_body)
    int B, ld;
    float inv_bk, reg_c;
};
__device__ __forceinline__ NceTerms nce_terms(const float* lse, const float* mean, int B, int K, int ld, float reg) {
    return {lse, mean, B, ld, 1.f / ((float)B * (float)K), 2.f * reg / ((float)B * (float)B * (float)K)};
}

// every row is a candidate of every column
struct NceDense : NceTerms {
    static constexpr bool live = true, own = true;
    __device__ __forceinline__ void column(int, int) {}
    __device__ __forceinline__ float dsp(int k, int b, int bp, float sp) const {
        float dsp = expf(sp - lse[k * B + bp]) * inv_bk + reg_c * mean[(long long)b * ld + bp];
        if (b == bp) dsp -= inv_bk;
        return dsp;
    }
};

// One 32 x 32 tile of (b, b') pairs of step k = blockIdx.z per workgroup, one thread per pair and trip (blockDim = 32 x 8, 4 rows per
// thread): rows b0 + 0..31 of the B score rows that start at row row0 of S and dS (k B, or the slot's first row in the ring of the
// banked loss), columns 32 blockIdx.x + 0..31.  Writes dS[row0 + b][b'] and, for a tile of the current batch, dST[k][b'][b] through
// LDS (storage dtype T).  Both stores write the zeros of the pad columns [B, ld) as well: the grids have ceil(ld / 32) tiles per
// side and the fast index of either store is bounded by ld, not by B — where ld reaches into a tile of its own (B = 32, ld = 39)
// that tile holds no pair at all and exists for those zeros.
// The loss scalars (nce_finalize_body) depend on the partials of the launches before this one only, so workgroup (0, 0, 0) also
// does that reduction: no launch of its own.
template <typename T, typename P>
__device__ __forceinline__ void nce_grad_tile(const float* __restrict__ S, T* __restrict__ dS, T* __restrict__ dST, int B, int K, int ld,
                                              int softplus, float reg, long long row0, int b0, P pol, const float* __restrict__ colp,
                                              int ncol, const float* __restrict__ pairp, int npair, float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // ty 0..7
    const int bp0 = blockIdx.x * 32, bp = bp0 + tx;
    const int k = blockIdx.z;
    pol.column(k, bp);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = b0 + ty + 8 * r;
        float g = 0.f;
        if (pol.live && b < B && bp < B) {
            const float x = S[(row0 + b) * ld + bp];
            const float sp = score_tf(x, softplus);
            g = pol.dsp(k, b, bp, sp) * score_grad(x, softplus);
        }
        if (b < B && bp < ld) dS[(row0 + b) * ld + bp] = from_f32<T>(g);
        tile[ty + 8 * r][tx] = g;
    }
    if (pol.own) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int bq = bp0 + ty + 8 * r, b = b0 + tx;
            if (b < ld && bq < B) dST[((long long)k * B + bq) * ld + b] = from_f32<T>(tile[tx][ty + 8 * r]);
        }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) nce_finalize_body(colp, ncol, pairp, npair, out, B, K, reg);
}

// grid (ceil(ld / 32), ceil(ld / 32), K)
template <typename T>
__global__ __launch_bounds__(256) void nce_grad_kernel(const float* __restrict__ S, const float* __restrict__ lse,
                                                       const float* __restrict__ mean, T* __restrict__ dS, T* __restrict__ dST,
                                                       int B, int K, int ld, int softplus, float reg, const float* __restrict__ colp,
                                                       int ncol, const float* __restrict__ pairp, int npair, float* __restrict__ out) {
    const int k = blockIdx.z;
    nce_grad_tile<T>(S, dS, dST, B, K, ld, softplus, reg, (long long)k * B, blockIdx.y * 32,
                     NceDense{nce_terms(lse, mean, B, K, ld, reg)}, colp, ncol, pairp, npair, out);
}

// score_over_all_timesteps=True branch (contrastive_estimation_training.py:108-114, :141): S is the full R x R score
// matrix, R = B*K, row r = (b,k) a prediction, column c = (b',k') a target.  lse[c] (over ALL rows) comes from
// nce_col_kernel(K=1, B=R).  Gradient w.r.t. the linear scores:
//   dsp[r][c] = (exp(sp[r][c] - lse[c]) - [r == c]) / R + 2 reg / (B B K K) * m[b][c],   m[b][c] = mean_k sp[(b,k)][c]
// The kernel is element-wise given lse, so it runs once on S (writing dS) and once on S^T (writing dS^T) with the
// roles of the two strides swapped — no transposes.  Element (r=(b,k), c) of the input sits at c*sc + (b*K+k)*sr.
// FAST_C: consecutive threads walk c (S, sc = 1) or b (S^T, sr = 1; a thread then owns K contiguous elements).
// KT > 0: K as a compile-time constant — the K scores of a pair are loaded once, all loads in flight (with a run-time K the
// pair's 2 K dependent-latency loads made the launch latency-bound: 85 us for 38 MB at B = 256, K = 12).
template <typename T, bool FAST_C, int KT>
__global__ __launch_bounds__(256) void nce_all_grad_kernel(const float* __restrict__ S, const float* __restrict__ lse,
                                                           T* __restrict__ dS, float* __restrict__ partial, int B, int K_rt,
                                                           long long sc, long long sr, int softplus, float reg,
                                                           int want_partials) {
    __shared__ float red[3][256];
    const int K = KT > 0 ? KT : K_rt;
    const int R = B * K;
    const long long total = (long long)B * R;                 // (b, c) pairs
    const float inv_r = 1.f / (float)R;
    const float reg_c = 2.f * reg / ((float)B * (float)B * (float)K * (float)K);
    float valid = 0.f, msq = 0.f, mx = -INFINITY;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int b = FAST_C ? (int)(idx / R) : (int)(idx % B);
        const int c = FAST_C ? (int)(idx % R) : (int)(idx / B);
        const float* base = S + (long long)c * sc + (long long)b * K * sr;
        float m = 0.f;
        const float l = lse[c];
        T* obase = dS + (long long)c * sc + (long long)b * K * sr;
        if (KT > 0) {
            float raw[KT > 0 ? KT : 1], spv[KT > 0 ? KT : 1];
#pragma unroll
            for (int k = 0; k < KT; ++k) raw[k] = base[(long long)k * sr];
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                spv[k] = score_tf(raw[k], softplus);
                m += spv[k];
                mx = fmaxf(mx, spv[k]);
                if (b * K + k == c) valid += spv[k];
            }
            m /= (float)K;
            msq += m * m;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                float dsp = expf(spv[k] - l) * inv_r + reg_c * m;
                if (b * K + k == c) dsp -= inv_r;
                obase[(long long)k * sr] = from_f32<T>(dsp * score_grad(raw[k], softplus));
            }
            continue;
        }
        for (int k = 0; k < K; ++k) {
            const float sp = score_tf(base[(long long)k * sr], softplus);
            m += sp;
            mx = fmaxf(mx, sp);
            if (b * K + k == c) valid += sp;
        }
        m /= (float)K;
        msq += m * m;
        for (int k = 0; k < K; ++k) {
            const float x = base[(long long)k * sr];
            const float sp = score_tf(x, softplus);
            float dsp = expf(sp - l) * inv_r + reg_c * m;
            if (b * K + k == c) dsp -= inv_r;
            obase[(long long)k * sr] = from_f32<T>(dsp * score_grad(x, softplus));
        }
    }
    if (!want_partials) return;
    block_reduce<3, 2>(red, {valid, msq, mx});
    if (threadIdx.x == 0) {
        partial[blockIdx.x * 3 + 0] = red[0][0];
        partial[blockIdx.x * 3 + 1] = red[1][0];
        partial[blockIdx.x * 3 + 2] = red[2][0];
    }
}

// all-timesteps finalize: out[0] = loss, out[1] = max score, out[2] = -mean valid, out[3] = mean lse, out[4] = reg term
__global__ __launch_bounds__(256) void nce_all_finalize_kernel(const float* __restrict__ col_partial, int ncol, const float* __restrict__ grad_partial,
                                        int ngrad, float* __restrict__ out, int B, int K, float reg) {
    // fixed-shape tree reduction: the summation order depends only on (ncol, ngrad), not on timing
    __shared__ float red[4][256];
    float lse_sum = 0.f, valid = 0.f, msq = 0.f, mx = -INFINITY;
    for (int i = threadIdx.x; i < ncol; i += 256) lse_sum += col_partial[i];
    for (int i = threadIdx.x; i < ngrad; i += 256) {
        valid += grad_partial[i * 3 + 0];
        msq += grad_partial[i * 3 + 1];
        mx = fmaxf(mx, grad_partial[i * 3 + 2]);
    }
    block_reduce<4, 3>(red, {lse_sum, valid, msq, mx});
    if (threadIdx.x != 0) return;
    lse_sum = red[0][0]; valid = red[1][0]; msq = red[2][0]; mx = red[3][0];
    const float r = (float)B * (float)K;
    const float t_valid = -valid / r, t_lse = lse_sum / r, t_reg = reg * msq / ((float)B * (float)B * (float)K);
    out[0] = t_valid + t_lse + t_reg;
    out[1] = mx;
    out[2] = t_valid;
    out[3] = t_lse;
    out[4] = t_reg;
    // NaN guard of the reference (contrastive_estimation_training.py:124-133: isnan of the loss BEFORE the regulariser, then
    // `return` before backward() / optimizer.step()): out[5] = this step's indicator, out[6] = sticky (stays raised until the host
    // clears it) — cpc_adam / cpc_adam_dev skip their update while it is raised
    const float lb = t_valid + t_lse;
    const float bad = (lb != lb) ? 1.f : 0.f;
    out[5] = bad;
    if (bad != 0.f) out[6] = 1.f;
}

// ---- validation quantities (ContrastiveEstimationTrainer.validate, contrastive_estimation_training.py:227-247) ----
// One wave per score row: sum of the transformed scores, first arg max over the row's columns, and the row's "valid" score
// (the column `diag`).  Default branch: row r = (k, b) of S[k][b][b'], diag = b; all-timesteps branch: row r = (b, k) of the
// R x R matrix, diag = r.
__global__ __launch_bounds__(256) void nce_row_eval_kernel(const float* __restrict__ S, int rows, int cols, int ld, int diag_mod,
                                                           int softplus, float* __restrict__ rsum, int* __restrict__ rarg,
                                                           float* __restrict__ rvalid) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* row = S + (long long)r * ld;
    float sum = 0.f, best = -INFINITY;
    int arg = 0x7fffffff;                                     // (a lane without columns keeps it: it loses every comparison below)
    for (int c = lane; c < cols; c += 64) {
        const float v = score_tf(row[c], softplus);
        sum += v;
        if (c == lane || v > best || (v != v && best == best)) { best = v; arg = c; }      // a NaN wins, as in torch.argmax
    }
    // first arg max, as torch.argmax: a NaN beats every number, and between two NaNs or two equal numbers the smaller column wins
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        sum += __shfl_xor(sum, o, 64);
        const bool onan = ob != ob, bnan = best != best;
        const bool take = onan ? (!bnan || oa < arg) : (!bnan && (ob > best || (ob == best && oa < arg)));
        if (take) { best = ob; arg = oa; }
    }
    if (lane == 0) {
        rsum[r] = sum;
        rarg[r] = arg;
        rvalid[r] = score_tf(row[diag_mod > 0 ? r % diag_mod : r], softplus);
    }
}

// out[0..K) (+)= per-step losses, out[K..2K) (+)= per-step accuracies, out[2K] (+)= mean score of this batch.
// Default branch: the reference forms noise = logsumexp(s.view(-1, B, K), 0) from the CONTIGUOUS (b, k, b') tensor, i.e. it
// reads the (k, b') array of column log-sum-exps as a (B, K) matrix in flat order, and averages
// valid[j][l] - noise[j][l] over j: lse[j*K + l] with lse stored flat as [k*B + b'].
__global__ __launch_bounds__(256) void nce_eval_finalize_kernel(const float* __restrict__ lse, const float* __restrict__ rsum,
                                                                const int* __restrict__ rarg, const float* __restrict__ rvalid,
                                                                float* __restrict__ out, int B, int K, int all_t, int accumulate) {
    __shared__ float red[1][256];
    const int R = B * K;
    for (int k = 0; k < K; ++k) {
        float dl = 0.f, hit = 0.f;
        for (int j = threadIdx.x; j < B; j += 256) {
            if (all_t) {
                const int r = j * K + k;
                dl += rvalid[r] - lse[r];
                hit += rarg[r] == r ? 1.f : 0.f;
            } else {
                dl += rvalid[k * B + j] - lse[j * K + k];
                hit += rarg[k * B + j] == j ? 1.f : 0.f;
            }
        }
        block_reduce<1>(red, {dl});
        const float loss_k = -red[0][0] / (float)B;
        __syncthreads();
        block_reduce<1>(red, {hit});
        const float acc_k = red[0][0] / (float)(all_t ? R : B);
        __syncthreads();
        if (threadIdx.x == 0) {
            out[k] = (accumulate ? out[k] : 0.f) + loss_k;
            out[K + k] = (accumulate ? out[K + k] : 0.f) + acc_k;
        }
    }
    float tot = 0.f;
    for (int r = threadIdx.x; r < R; r += 256) tot += rsum[r];
    block_reduce<1>(red, {tot});
    if (threadIdx.x == 0) {
        const float mean = red[0][0] / ((float)R * (float)(all_t ? R : B));
        out[2 * K] = (accumulate ? out[2 * K] : 0.f) + mean;
    }
}

// ---- score_over_all_timesteps = True with the column pass fused into the score GEMM (bf16; launch_score_lse in gemm.hip) ----
// The GEMM leaves, per M tile and column, the online log-sum-exp pair (pm, ps) = (max, sum exp(s - max)) of the LINEAR scores s over
// the tile's 256 rows.  For softplus scores exp(softplus(s)) = 1 + exp(s) (torch's threshold 20 changes that by < e^-20), so
//   lse[c] = log( [softplus] * nrows + sum_tiles ps * exp(pm) )
// needs no softplus at all.  colp[block] = {sum of the block's lse, max of its pm}.
__global__ __launch_bounds__(256) void nce_lse_merge_kernel(const float* __restrict__ pm, const float* __restrict__ ps, int nparts, int ncols,
                                                            int softplus, float nrows, float* __restrict__ lse, float* __restrict__ colp) {
    __shared__ float red[2][256];
    const int c = blockIdx.x * 256 + threadIdx.x;
    float l = 0.f, mx = -INFINITY;
    if (c < ncols) {
        for (int i = 0; i < nparts; ++i) mx = fmaxf(mx, pm[(long long)i * ncols + c]);
        const float ref = softplus ? fmaxf(mx, 0.f) : mx;
        float tot = softplus ? nrows * expf(-ref) : 0.f;
        for (int i = 0; i < nparts; ++i) tot += ps[(long long)i * ncols + c] * expf(pm[(long long)i * ncols + c] - ref);
        l = ref + logf(tot);
        lse[c] = l;
    }
    block_reduce<2, 1>(red, {l, mx});
    if (threadIdx.x == 0) {
        colp[blockIdx.x * 2] = red[0][0];
        colp[blockIdx.x * 2 + 1] = red[1][0];
    }
}

// d loss / d linear score from the f32 scores the fused GEMM stored, and its transpose: Sb [items K][ld] (row (b, k) = a prediction, column
// c = a target), lse [ncols]:
//   dS[r][c] = score'(s) * ( (exp(sp - lse[c]) - [c == r + diag_off]) / n_rows + 2 reg / (n_items^2 K^2) * m[b][c] ),   m = mean_k sp[(b,k)][c]
// (n_rows / n_items: of the WHOLE problem — a rank of a data-parallel run holds a strip of it).  Workgroup = 16 items x 64 columns, 256 threads:
// thread = (item, 4 columns), 16-byte loads / 8-byte stores along the rows; the transposed copy goes through an LDS image [64][16 K] and leaves
// as 16 K contiguous elements per column.  gradp[block] = sum of m^2 over the block's (item, column) pairs (the regulariser's value).
constexpr int NFG_IT = 16, NFG_CW = 64;
// KT > 0: K as a compile-time constant — the K rows of a thread are loaded once, all loads in flight (with a run-time K the rows are read
// twice, one dependent load after the other: 117 us instead of 3x us for the 38 MB of B = 256, K = 12).
template <int KT>
__global__ __launch_bounds__(256) void nce_fused_grad_kernel(const float* __restrict__ Sb, const float* __restrict__ lse, bf16_t* __restrict__ dS,
                                                             bf16_t* __restrict__ dST, float* __restrict__ gradp, int items, int K_rt, int ncols,
                                                             long long ld, long long ldT, int diag_off, int softplus, float inv_r, float reg_c) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tsm[];
    __shared__ float red[1][256];
    const int K = KT > 0 ? KT : K_rt;
    const int rs = NFG_IT * K * 2 + 16;                       // LDS image row stride (bytes): one column's 16 K gradients + pad
    const int tid = threadIdx.x, cg = tid & 15, it = tid >> 4;          // thread = (item, 4 columns)
    const int c0 = blockIdx.x * NFG_CW + cg * 4, item = blockIdx.y * NFG_IT + it;
    const bool on = item < items && c0 < ncols;
    float msq = 0.f;
    if (on) {
        const f32x4 l4 = *(const f32x4*)(lse + c0);
        f32x4 m4 = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* src = Sb + (long long)item * K * ld + c0;
        bf16_t* dst = dS + (long long)item * K * ld + c0;
        const int r0 = item * K + diag_off;                    // the column of row (item, 0)'s own target
        f32x4 v[KT > 0 ? KT : 1];
        if constexpr (KT > 0) {
#pragma unroll
            for (int k = 0; k < KT; ++k) v[k] = *(const f32x4*)(src + (long long)k * ld);
#pragma unroll
            for (int k = 0; k < KT; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) m4[e] += score_tf(v[k][e], softplus);
        } else {
            for (int k = 0; k < K; ++k) {
                const f32x4 x = *(const f32x4*)(src + (long long)k * ld);
#pragma unroll
                for (int e = 0; e < 4; ++e) m4[e] += score_tf(x[e], softplus);
            }
        }
        const float inv_k = 1.f / (float)K;
#pragma unroll
        for (int e = 0; e < 4; ++e) { m4[e] *= inv_k; msq += m4[e] * m4[e]; }
        auto grad4 = [&](const f32x4& x, int k) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float d = __expf(score_tf(x[e], softplus) - l4[e]) * inv_r + reg_c * m4[e];
                if (c0 + e == r0 + k) d -= inv_r;
                o[e] = (bf16_t)(d * score_grad(x[e], softplus));
            }
            return o;
        };
        auto pair = [&](const f32x4& xa, const f32x4& xb, int k) {
            const bf16x4 oa = grad4(xa, k), ob = grad4(xb, k + 1);
            *(bf16x4*)(dst + (long long)k * ld) = oa;
            *(bf16x4*)(dst + (long long)(k + 1) * ld) = ob;
            if (dST != nullptr) {
                // (element e of row k in the low half, of row k + 1 in the high half; taken from the packed words: hipcc 7.2 gave element 0
                // for every e when the elements were bit-cast one by one — tools/dbg_grad.py, three columns of four wrong)
                const uint2 ua = __builtin_bit_cast(uint2, oa), ub = __builtin_bit_cast(uint2, ob);
                const unsigned wa[2] = {ua.x, ua.y}, wb[2] = {ub.x, ub.y};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned lo = (wa[e >> 1] >> (16 * (e & 1))) & 0xffffu, hi = (wb[e >> 1] >> (16 * (e & 1))) & 0xffffu;
                    *(unsigned*)(tsm + (cg * 4 + e) * rs + (it * K + k) * 2) = lo | (hi << 16);          // image[column][row pair]
                }
            }
        };
        if constexpr (KT > 0) {
#pragma unroll
            for (int k = 0; k < KT; k += 2) pair(v[k], v[k + 1], k);
        } else {
            for (int k = 0; k < K; k += 2)
                pair(*(const f32x4*)(src + (long long)k * ld), *(const f32x4*)(src + (long long)(k + 1) * ld), k);
        }
    }
    if (dST != nullptr) {
        __syncthreads();
        // column cl of the tile: NFG_IT K contiguous elements of row c of dS^T, starting at element blockIdx.y NFG_IT K
        const int cpr = NFG_IT * K / 8;                       // 16-byte chunks per column
        const int rows_here = min(NFG_IT, items - (int)blockIdx.y * NFG_IT) * K;
        for (int q = tid; q < NFG_CW * cpr; q += 256) {
            const int cl = q / cpr, ch = q % cpr;
            const int c = blockIdx.x * NFG_CW + cl;
            if (c >= ncols || ch * 8 >= rows_here) continue;
            bf16_t* out = dST + (long long)c * ldT + (long long)blockIdx.y * NFG_IT * K + ch * 8;
            if (ch * 8 + 8 <= rows_here) {
                *(uint4*)out = *(const uint4*)(tsm + cl * rs + ch * 16);
            } else {                                          // partial last item block: the chunk's elements up to rows_here only
                for (int e = 0; e < rows_here - ch * 8; ++e) out[e] = ((const bf16_t*)(tsm + cl * rs + ch * 16))[e];
            }
        }
    }
    block_reduce<1>(red, {msq});
    if (tid == 0 && gradp != nullptr) gradp[blockIdx.y * gridDim.x + blockIdx.x] = red[0][0];
}

// Loss scalars of the fused path.  mode 0: reduce the partials and write out[0..6] (single process); mode 1: reduce only ->
// sums[0..3] = {sum of the valid scores, sum of lse, sum of m^2, max linear score} (a rank's share: all-reduce them, SUM / SUM / SUM / MAX);
// mode 2: out[0..6] from sums.  out as cpc_nce_loss_all writes it.
__global__ __launch_bounds__(256) void nce_fused_finalize_kernel(const float* __restrict__ colp, int ncolp, const float* __restrict__ valid, int nvalid,
                                                                 const float* __restrict__ gradp, int ngrad, float* __restrict__ sums, int mode,
                                                                 float n_rows, float n_items, int K, float reg, int softplus,
                                                                 float* __restrict__ out) {
    __shared__ float red[4][256];
    float sv = 0.f, sl = 0.f, sm = 0.f, mx = -INFINITY;
    if (mode != 2) {
        for (int i = threadIdx.x; i < nvalid; i += 256) sv += score_tf(valid[i], softplus);
        for (int i = threadIdx.x; i < ncolp; i += 256) { sl += colp[2 * i]; mx = fmaxf(mx, colp[2 * i + 1]); }
        for (int i = threadIdx.x; i < ngrad; i += 256) sm += gradp[i];
        block_reduce<4, 3>(red, {sv, sl, sm, mx});
        sv = red[0][0]; sl = red[1][0]; sm = red[2][0]; mx = red[3][0];
    } else {
        sv = sums[0]; sl = sums[1]; sm = sums[2]; mx = sums[3];
    }
    if (threadIdx.x != 0) return;
    if (mode == 1) {
        sums[0] = sv; sums[1] = sl; sums[2] = sm; sums[3] = mx;
        return;
    }
    const float t_valid = -sv / n_rows, t_lse = sl / n_rows, t_reg = reg * sm / (n_items * n_rows);
    out[0] = t_valid + t_lse + t_reg;
    out[1] = score_tf(mx, softplus);
    out[2] = t_valid;
    out[3] = t_lse;
    out[4] = t_reg;
    const float lb = t_valid + t_lse;             // the reference's NaN guard tests the loss before the regulariser (:124)
    const float bad = (lb != lb) ? 1.f : 0.f;
    out[5] = bad;
    if (bad != 0.f) out[6] = 1.f;
}

// ---- sampled negatives: the equal-step loss over N seeded negatives per target (include/cpc_hip.h, cpc_nce_loss_sampled) ----
// Every target column (k, b') keeps its own row b' and the N rows b != b' with the smallest (key, b), key a counter-based hash of
// (seed, draw, k, b', b) with the arithmetic of drop_hash (attn.hip).  Nothing of size K B B is stored: the column pass finds each
// column's N-th smallest composite (key << 32 | b) and leaves it as a threshold, the gradient pass recomputes an element's key and
// compares.  ONE WAVE PER COLUMN, a lane holding rows lane, lane + 64, ...: the N-th smallest is found bit by bit from the top
// (count of keys <= candidate through ballots, 32 steps; then 10 steps over the row index among the rows that tie with the
// threshold key), i.e. 42 x ceil(B / 64) wave-wide compares per column and neither LDS nor a barrier — rank counting costs B^2 / 64
// = 1024 wave-wide 64-bit compares per column at B = 256, an LDS bitonic sort 36 barrier-separated stages.
constexpr int NSM_MAXB = 1024;      // 16 rows per lane; the row index takes the low 10 bits of the tie search
constexpr int NSM_COLS = 4;         // columns (waves) per workgroup of the column pass
constexpr unsigned long long NSM_DRAW = 0x632BE59BD9B4E019ull, NSM_STEP = 0x9E3779B97F4A7C15ull, NSM_IDX = 0xD1B54A32D192ED03ull;

// what a column's keys share: seed + NSM_DRAW draw + NSM_STEP (k + 1) + (b' B) NSM_IDX   (mod 2^64)
__device__ __forceinline__ unsigned long long nsm_col_base(unsigned long long seed, unsigned long long draw, int k, int bp, int B) {
    return seed + NSM_DRAW * draw + NSM_STEP * (unsigned long long)(k + 1) + (unsigned long long)bp * (unsigned long long)B * NSM_IDX;
}
__device__ __forceinline__ unsigned nsm_key(unsigned long long col_base, int b) {
    unsigned long long z = col_base + (unsigned long long)b * NSM_IDX;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned)(z >> 32);
}

// The search of every selection: called by all 64 lanes of a wave with key[h] of row lane + 64 h and ok bit h set where that row takes
// part; returns the n-th smallest composite (key << 32 | row) among the rows that take part (1 <= n <= their number).
template <int H>
__device__ __forceinline__ unsigned long long nsm_search(unsigned ok, int lane, int n, const unsigned (&key)[H]) {
    unsigned tk = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = tk | ((1u << bit) - 1u);
        int cnt = 0;
#pragma unroll
        for (int h = 0; h < H; ++h) cnt += __popcll(__ballot(((ok >> h) & 1u) && key[h] <= cand));
        if (cnt < n) tk |= 1u << bit;
    }
    int below = 0;
#pragma unroll
    for (int h = 0; h < H; ++h) below += __popcll(__ballot(((ok >> h) & 1u) && key[h] < tk));
    const int need = n - below;                 // >= 1 rows with key == tk belong, the ones with the smallest index
    unsigned tb = 0;
    for (int bit = 9; bit >= 0; --bit) {
        const unsigned cand = tb | ((1u << bit) - 1u);
        int cnt = 0;
#pragma unroll
        for (int h = 0; h < H; ++h) cnt += __popcll(__ballot(((ok >> h) & 1u) && key[h] == tk && (unsigned)(lane + 64 * h) <= cand));
        if (cnt < need) tb |= 1u << bit;
    }
    return ((unsigned long long)tk << 32) | tb;
}

// ---- grouped negatives: the same chain with candidates restricted by a per-item group id (include/cpc_hip.h, cpc_nce_loss_grouped) ----
// Row b is ELIGIBLE for column (k, b') when b != b' and (groups[b] == groups[b']) == (mode == same); the column keeps its own row and
// the n = min(n_neg, |Elig|) eligible rows with the smallest (key, b) (n_neg == 0: all of them).  A sampled draw is a grouped draw
// with one group and mode "same", so everything below is written once, GROUPED a compile-time flag: without it every other row is
// eligible, and no instantiation reads `groups` or `mode`.  Eligibility is one more condition on the ok bits of the selection and is
// tested AGAIN, before the threshold, wherever membership is asked: a column whose eligible set is empty needs no sentinel threshold.
constexpr unsigned long long NSM_ALL = ~0ull;       // threshold of a column that keeps every eligible row (no composite reaches it: row < 1024)

__device__ __forceinline__ bool nsg_eligible(int g, int gp, int mode) { return (g == gp) == (mode == 0); }

// The selection routine of every entry point.  Called by all 64 lanes of a wave for column (k, b').  ok bit h <- row lane + 64 h is
// eligible; returns the column's threshold, the n-th smallest composite among the eligible rows.  |Elig| is B - 1 or comes from
// ballots; with n == |Elig| (always when n_neg == 0, for an empty set, and for n_neg == B - 1 sampled negatives) nothing is hashed or
// searched, the threshold is NSM_ALL and the keys are zero: the branch is wave-uniform.
template <bool GROUPED, int H>
__device__ __forceinline__ unsigned long long nsm_select(const int* __restrict__ groups, int mode, unsigned long long seed,
                                                         unsigned long long draw, int k, int lane, int bp, int B, int n_neg,
                                                         unsigned (&key)[H], unsigned& ok_out) {
    int gp = 0;
    if constexpr (GROUPED) gp = groups[bp];
    unsigned ok = 0;
    int elig = GROUPED ? 0 : B - 1;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int row = lane + 64 * h;
        bool e = row < B && row != bp;
        if constexpr (GROUPED) {
            e = e && nsg_eligible(groups[row < B ? row : 0], gp, mode);
            elig += __popcll(__ballot(e));
        }
        if (e) ok |= 1u << h;
    }
    ok_out = ok;
    const int n = (n_neg == 0 || n_neg > elig) ? elig : n_neg;
    if (n == elig) {
#pragma unroll
        for (int h = 0; h < H; ++h) key[h] = 0;
        return NSM_ALL;
    }
    const unsigned long long base = nsm_col_base(seed, draw, k, bp, B);
#pragma unroll
    for (int h = 0; h < H; ++h) key[h] = nsm_key(base, lane + 64 * h);
    return nsm_search<H>(ok, lane, n, key);
}

// The membership test of every entry point: row b < B is a candidate of column b' with threshold t when it is the column's own row,
// or is eligible and its composite is within the threshold (NSM_ALL admits every key).  No branch in it: the four rows of a gradient
// thread hash side by side.
__device__ __forceinline__ bool nsm_member(int b, int bp, bool eligible, unsigned long long t, unsigned key) {
    return b == bp || (eligible && (((unsigned long long)key << 32) | (unsigned)b) <= t);
}

// Column pass of one wave: threshold of column col = k B + b', and the log-sum-exp over its candidates.  The wave-wide max and sum
// are xor butterflies (every lane ends with the same bits), the lane's own sum runs over h in order: nothing depends on timing.
template <bool GROUPED, int H>
__device__ __forceinline__ void nsm_col_body(const float* __restrict__ S, unsigned long long* __restrict__ thr, float* __restrict__ lse,
                                             int B, int ld, int softplus, const int* __restrict__ groups, int mode, int n_neg,
                                             unsigned long long seed, unsigned long long draw, int col) {
    const int lane = threadIdx.x & 63;
    const int k = col / B, bp = col % B;
    const float* cp = S + (long long)k * B * ld + bp;
    float v[H];
    unsigned key[H];
#pragma unroll
    for (int h = 0; h < H; ++h) v[h] = (lane + 64 * h < B) ? cp[(long long)(lane + 64 * h) * ld] : 0.f;      // in flight during the selection
    unsigned ok;
    const unsigned long long t = nsm_select<GROUPED, H>(groups, mode, seed, draw, k, lane, bp, B, n_neg, key, ok);
    float mx = -INFINITY;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int row = lane + 64 * h;
        const bool in = row < B && nsm_member(row, bp, (ok >> h) & 1u, t, key[h]);
        v[h] = in ? score_tf(v[h], softplus) : -INFINITY;
        mx = fmaxf(mx, v[h]);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
#pragma unroll
    for (int h = 0; h < H; ++h)                  // a NaN score: dropped by fmaxf, carried by the sum, as nce_col_body does
        sum += (v[h] == mx) ? 1.f : expf(v[h] - mx);          // (the max itself is 1 also when it is +inf: inf - inf would be NaN)
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) {
        thr[col] = t;
        lse[col] = mx + logf(sum);
    }
}

// Column pass + pair means in ONE launch, as nce_col_mean_kernel: the first ncb workgroups take NSM_COLS columns each, the rest the
// pairs (nce_mean_body: the regulariser, the max score and the valid scores run over ALL scores and do not know about the sampling).
template <bool GROUPED, int KT, int H>
__global__ __launch_bounds__(256) void nce_selected_col_mean_kernel(const float* __restrict__ S, unsigned long long* __restrict__ thr,
                                                                    float* __restrict__ lse, float* __restrict__ mean,
                                                                    float* __restrict__ pairp, int B, int K, int ld, int softplus,
                                                                    const int* __restrict__ groups, int mode, int n_neg,
                                                                    unsigned long long seed, unsigned long long draw, int ncb) {
    if ((int)blockIdx.x < ncb) {
        const int col = blockIdx.x * NSM_COLS + (threadIdx.x >> 6);
        if (col < K * B) nsm_col_body<GROUPED, H>(S, thr, lse, B, ld, softplus, groups, mode, n_neg, seed, draw, col);     // (wave-uniform)
    } else {
        nce_mean_body<KT>(S, mean, pairp, B, K, ld, softplus, blockIdx.x - ncb, (long long)B * ld);
    }
}

// exp(sp - lse) only where row b is a candidate of column (k, b'): the element's eligibility and key are computed again and compared
// with the threshold the column pass left.
template <bool GROUPED>
struct NceSelected : NceTerms {
    static constexpr bool live = true, own = true;
    const unsigned long long* thr;
    const int* groups;
    int mode;
    unsigned long long seed, draw;
    unsigned long long base, t;         // of the thread's column, set by column(): what its keys share, its threshold,
    float l;                            // its log-sum-exp
    int gp;                             // and its group
    __device__ __forceinline__ void column(int k, int bp) {
        base = nsm_col_base(seed, draw, k, bp, B);
        t = bp < B ? thr[k * B + bp] : 0ull;
        l = bp < B ? lse[k * B + bp] : 0.f;
        if constexpr (GROUPED) gp = bp < B ? groups[bp] : 0;
    }
    __device__ __forceinline__ float dsp(int k, int b, int bp, float sp) const {
        float dsp = reg_c * mean[(long long)b * ld + bp];
        bool eligible = true;
        if constexpr (GROUPED) eligible = nsg_eligible(groups[b], gp, mode);
        unsigned key = 0;           // (grouped: the hash is spared where the answer does not hang on it; sampled rows hash always)
        if (!GROUPED || (eligible && t != NSM_ALL)) key = nsm_key(base, b);
        if (nsm_member(b, bp, eligible, t, key)) dsp += expf(sp - l) * inv_bk;
        if (b == bp) dsp -= inv_bk;
        return dsp;
    }
};

// grid as nce_grad_kernel's; the column sums of the loss scalars are the K B log-sum-exps themselves, in nce_finalize_body's fixed order
template <typename T, bool GROUPED>
__global__ __launch_bounds__(256) void nce_selected_grad_kernel(const float* __restrict__ S, const float* __restrict__ lse,
                                                                const unsigned long long* __restrict__ thr, const float* __restrict__ mean,
                                                                T* __restrict__ dS, T* __restrict__ dST, int B, int K, int ld, int softplus,
                                                                float reg, const int* __restrict__ groups, int mode, unsigned long long seed,
                                                                unsigned long long draw, const float* __restrict__ pairp, int npair,
                                                                float* __restrict__ out) {
    const int k = blockIdx.z;
    nce_grad_tile<T>(S, dS, dST, B, K, ld, softplus, reg, (long long)k * B, blockIdx.y * 32,
                     NceSelected<GROUPED>{nce_terms(lse, mean, B, K, ld, reg), thr, groups, mode, seed, draw}, lse, K * B, pairp, npair, out);
}

// mask[k][b][b'] = 1 where row b is a candidate of column (k, b') (its own row included), from the same selection routine.
template <bool GROUPED, int H>
__global__ __launch_bounds__(256) void nce_select_mask_kernel(unsigned char* __restrict__ mask, const int* __restrict__ groups, int B, int K,
                                                              int mode, int n_neg, unsigned long long seed, unsigned long long draw) {
    const int col = blockIdx.x * NSM_COLS + (threadIdx.x >> 6);
    if (col >= K * B) return;                   // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int k = col / B, bp = col % B;
    unsigned key[H];
    unsigned ok;
    const unsigned long long t = nsm_select<GROUPED, H>(groups, mode, seed, draw, k, lane, bp, B, n_neg, key, ok);
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int row = lane + 64 * h;
        if (row < B) mask[((long long)k * B + row) * B + bp] = nsm_member(row, bp, (ok >> h) & 1u, t, key[h]) ? 1 : 0;
    }
}

// ---- negative bank: the equal-step loss with the predictions of earlier steps as further candidates (include/cpc_hip.h, cpc_nce_loss_banked) ----
// S[k][r][b'], r = slot B + b over `slots` ring slots of B rows; a column's log-sum-exp runs over the rows of the valid slots (up to
// 64 B of them), everything else of the loss over slot `cur` alone.  Three launches: partial pass + pair means, merge, gradients.
// Partial pass: a wave takes NBK_CHUNK rows of one slot and 64 columns, lanes along b' (every row read is one coalesced 256-byte
// line), each lane an online (max, sum exp) pair in f32 over the chunk's rows in row order; a chunk never spans two slots, and the
// chunks of invalid slots are neither read nor written.  Merge: one thread per column over the chunks of the valid slots in chunk
// order.  Neither depends on the grid: the chunk constant alone fixes the summation order.
constexpr int NBK_CHUNK = 32;       // rows per (max, sum) pair
constexpr int NBK_WAVES = 4;        // chunks (waves) per workgroup of the partial pass

__host__ __device__ __forceinline__ bool nbk_valid(unsigned long long valid, int slot) { return (valid >> slot) & 1ull; }

// grid: npart = K x ceil(slots cps / NBK_WAVES) x ceil(B / 64) workgroups for the chunks (cps = ceil(B / NBK_CHUNK) chunks per slot),
// then the pair means of slot cur (nce_mean_body), in one launch as nce_col_mean_kernel.  part[chunk][k][b'] = (max, sum).
template <int KT>
__global__ __launch_bounds__(256) void nce_bank_partial_mean_kernel(const float* __restrict__ S, float2* __restrict__ part,
                                                                    float* __restrict__ mean, float* __restrict__ pairp, int B, int K,
                                                                    int ld, int slots, int cur, unsigned long long valid, int softplus,
                                                                    int cps, int ncb, int npart) {
    if ((int)blockIdx.x >= npart) {
        nce_mean_body<KT>(S + (long long)cur * B * ld, mean, pairp, B, K, ld, softplus, blockIdx.x - npart, (long long)slots * B * ld);
        return;
    }
    const int ngrp = (slots * cps + NBK_WAVES - 1) / NBK_WAVES;
    const int cb = blockIdx.x % ncb, grp = (blockIdx.x / ncb) % ngrp, k = blockIdx.x / (ncb * ngrp);
    const int chunk = grp * NBK_WAVES + (threadIdx.x >> 6), bp = cb * 64 + (threadIdx.x & 63);
    if (chunk >= slots * cps || bp >= B) return;
    const int slot = chunk / cps;
    if (!nbk_valid(valid, slot)) return;                       // (wave-uniform)
    const int r0 = (chunk % cps) * NBK_CHUNK, r1 = min(B, r0 + NBK_CHUNK);
    const float* col = S + ((long long)k * slots + slot) * B * ld + bp;
    float mx = -INFINITY, sum = 0.f;
    for (int base = r0; base < r1; base += 8) {                // eight rows per trip, their loads in flight together
        float vv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) vv[u] = (base + u < r1) ? col[(long long)(base + u) * ld] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (base + u < r1) {
                const float v = score_tf(vv[u], softplus);
                if (v > mx) { sum = sum * expf(mx - v) + 1.f; mx = v; }
                else sum += (v == mx) ? 1.f : expf(v - mx);    // (a NaN score stays in the sum; +inf twice counts twice)
            }
        }
    }
    part[((long long)chunk * K + k) * B + bp] = make_float2(mx, sum);
}

// lse[c] for column c = k B + b' from the chunks of the valid slots, in chunk order, and one partial sum of lse per 256 columns.
// A chunk whose scores are all NaN has max = -inf and sum = NaN: it is weighed like any other, so that the NaN reaches the loss.
__global__ __launch_bounds__(256) void nce_bank_merge_kernel(const float2* __restrict__ part, int nchunk, int cps,
                                                             unsigned long long valid, int ncols, float* __restrict__ lse,
                                                             float* __restrict__ colp) {
    __shared__ float red[1][256];
    const int c = blockIdx.x * 256 + threadIdx.x;
    float l = 0.f;
    if (c < ncols) {
        float m = -INFINITY;
        for (int z = 0; z < nchunk; ++z)
            if (nbk_valid(valid, z / cps)) m = fmaxf(m, part[(long long)z * ncols + c].x);
        float tot = 0.f;
        for (int z = 0; z < nchunk; ++z) {
            if (!nbk_valid(valid, z / cps)) continue;
            const float2 p = part[(long long)z * ncols + c];
            tot += (p.x == m) ? p.y : p.y * expf(p.x - m);      // (p.x == m: as in nce_col_body, m = +inf included)
        }
        l = m + logf(tot);
        lse[c] = l;
    }
    block_reduce<1>(red, {l});
    if (threadIdx.x == 0) colp[blockIdx.x] = red[0][0];
}

// The ring's rows: a row of an invalid slot gets zero coefficients (written every launch), a row of a stale slot the softmax term
// alone, a row of slot cur also the diagonal and the regulariser, and its tile alone goes into dST_cur.
struct NceBanked : NceTerms {
    bool live, own;
    __device__ __forceinline__ void column(int, int) {}
    __device__ __forceinline__ float dsp(int k, int b, int bp, float sp) const {
        float dsp = expf(sp - lse[k * B + bp]) * inv_bk;
        if (own) {
            dsp += reg_c * mean[(long long)b * ld + bp];
            if (b == bp) dsp -= inv_bk;
        }
        return dsp;
    }
};

// grid (column tiles, slots x row tiles, K), ceil(ld / 32) tiles per side and slot as nce_grad_kernel's: a tile lies inside ONE slot
template <typename T>
__global__ __launch_bounds__(256) void nce_bank_grad_kernel(const float* __restrict__ S, const float* __restrict__ lse,
                                                            const float* __restrict__ mean, T* __restrict__ dS, T* __restrict__ dST,
                                                            int B, int K, int ld, int slots, int cur, unsigned long long valid,
                                                            int softplus, float reg, const float* __restrict__ colp, int ncol,
                                                            const float* __restrict__ pairp, int npair, float* __restrict__ out) {
    const int nrt = (ld + 31) / 32;
    const int slot = blockIdx.y / nrt, k = blockIdx.z;
    nce_grad_tile<T>(S, dS, dST, B, K, ld, softplus, reg, ((long long)k * slots + slot) * B, (blockIdx.y % nrt) * 32,
                     NceBanked{nce_terms(lse, mean, B, K, ld, reg), nbk_valid(valid, slot), slot == cur}, colp, ncol, pairp, npair, out);
}

}  // namespace

int launch_nce_lse_merge(const float* pm, const float* ps, int nparts, int ncols, int softplus, float nrows, float* lse, float* colp,
                         hipStream_t stream) {
    if (!pm || !ps || !lse || !colp || nparts <= 0 || ncols <= 0) return CPC_EINVAL;
    hipLaunchKernelGGL(nce_lse_merge_kernel, dim3((ncols + 255) / 256), dim3(256), 0, stream, pm, ps, nparts, ncols, softplus, nrows, lse, colp);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

long long nce_fused_grad_blocks(int items, int ncols) {
    return (long long)((ncols + NFG_CW - 1) / NFG_CW) * ((items + NFG_IT - 1) / NFG_IT);
}

int launch_nce_fused_grad(const void* Sb, const float* lse, void* dS, void* dST, float* gradp, int items, int K, int ncols, long long ld,
                          long long ldT, int diag_off, int softplus, float reg, float n_rows, float n_items, hipStream_t stream) {
    if (!Sb || !lse || !dS || items <= 0 || K < 2 || K % 2 || K > 24 || ncols <= 0 || ncols % 4 || ld % 8 || ld < ncols) return CPC_EINVAL;
    if (dST && (ldT % 8 || ldT < (long long)items * K)) return CPC_EINVAL;
    if ((uintptr_t)Sb % 16 || (uintptr_t)dS % 16 || (uintptr_t)dST % 16 || (uintptr_t)lse % 16) return CPC_EINVAL;
    const dim3 grid((ncols + NFG_CW - 1) / NFG_CW, (items + NFG_IT - 1) / NFG_IT);
    const size_t lds_bytes = dST ? (size_t)NFG_CW * (NFG_IT * K * 2 + 16) : 0;
    const float inv_r = 1.f / n_rows, reg_c = 2.f * reg / (n_items * n_items * (float)K * (float)K);
#define NFG_LAUNCH(KT) \
    hipLaunchKernelGGL(nce_fused_grad_kernel<KT>, grid, dim3(256), lds_bytes, stream, (const float*)Sb, lse, (bf16_t*)dS, (bf16_t*)dST, gradp, items, K, \
                       ncols, ld, ldT, diag_off, softplus, inv_r, reg_c)
    if (K == 12) NFG_LAUNCH(12); else if (K == 16) NFG_LAUNCH(16); else if (K == 8) NFG_LAUNCH(8); else NFG_LAUNCH(0);
#undef NFG_LAUNCH
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_nce_fused_finalize(const float* colp, int ncolp, const float* valid, int nvalid, const float* gradp, int ngrad, float* sums, int mode,
                              float n_rows, float n_items, int K, float reg, int softplus, float* out, hipStream_t stream) {
    if (mode < 0 || mode > 2 || (mode != 2 && (!colp || !valid || !gradp)) || (mode != 0 && !sums) || (mode != 1 && !out)) return CPC_EINVAL;
    if (mode != 2 && (ncolp < 0 || nvalid < 0 || ngrad < 0)) return CPC_EINVAL;       // (a negative count would read as an empty array: a caller's mistake, not a strip without rows)
    hipLaunchKernelGGL(nce_fused_finalize_kernel, dim3(1), dim3(256), 0, stream, colp, ncolp, valid, nvalid, gradp, ngrad, sums, mode, n_rows, n_items,
                       K, reg, softplus, out);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// workspace: lse [K][B] + column partials [K * ceil(B / NCE_CW)] + pair partials [3 * ceil(B*B/256)] + pair means [B][ld <= B + 7]
long long nce_workspace_floats(int B, int K) {
    const long long nmb = ((long long)B * B + 255) / 256;
    return (long long)K * B + (long long)K * ((B + NCE_CW - 1) / NCE_CW) + 3 * nmb + (long long)B * (B + 8);
}

int launch_nce(const float* S, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld, int softplus, float reg,
               int dtype, hipStream_t stream) {
    if (B <= 0 || K <= 0 || ld < B || ld > B + 7) return CPC_EINVAL;
    if (dtype != CPC_DTYPE_BF16 && dtype != CPC_DTYPE_F32) return CPC_EINVAL;       // before the first launch: a refused call writes nothing
    float* lse = workspace;
    const int ncb = (B + NCE_CW - 1) / NCE_CW;
    const int ncol = K * ncb;
    float* colp = lse + (long long)K * B;
    float* gradp = colp + ncol;
    const int nmb = (int)(((long long)B * B + 255) / 256);
    float* mean = gradp + 3LL * nmb;
    const int nb = (ld + 31) / 32;
    // two launches: column log-sum-exps + pair means, then gradients + loss scalars (each launch of this path is latency-bound)
    const dim3 g1(ncol + nmb);
    if (K == 12) hipLaunchKernelGGL(nce_col_mean_kernel<12>, g1, dim3(256), 0, stream, S, lse, colp, mean, gradp, B, K, ld, softplus, ncb);
    else if (K == 16) hipLaunchKernelGGL(nce_col_mean_kernel<16>, g1, dim3(256), 0, stream, S, lse, colp, mean, gradp, B, K, ld, softplus, ncb);
    else hipLaunchKernelGGL(nce_col_mean_kernel<0>, g1, dim3(256), 0, stream, S, lse, colp, mean, gradp, B, K, ld, softplus, ncb);
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((nce_grad_kernel<bf16_t>), dim3(nb, nb, K), dim3(256), 0, stream, S, lse, mean, (bf16_t*)dS, (bf16_t*)dST,
                           B, K, ld, softplus, reg, colp, ncol, gradp, nmb, out);
    else
        hipLaunchKernelGGL((nce_grad_kernel<float>), dim3(nb, nb, K), dim3(256), 0, stream, S, lse, mean, (float*)dS, (float*)dST, B, K,
                           ld, softplus, reg, colp, ncol, gradp, nmb, out);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// ---- sampled and grouped negatives ----
// workspace: thresholds [K][B] (64 bits each, first: the workspace must be 8-byte aligned) + lse [K][B] + pair partials
// [3 * ceil(B*B/256)] + pair means [B][ld <= B + 7].  (A threshold word is internal: a column that keeps every eligible row holds
// NSM_ALL instead of its largest composite — sampled negatives with n_neg == B - 1 included, which are not hashed or searched either.)
long long nce_sampled_workspace_floats(int B, int K) {
    if (B <= 0 || K <= 0) return 0;
    const long long nmb = ((long long)B * B + 255) / 256;
    return 3LL * K * B + 3 * nmb + (long long)B * (B + 8);
}
long long nce_grouped_workspace_floats(int B, int K) { return nce_sampled_workspace_floats(B, K); }

// The chain behind both entry points, which have checked their arguments: column pass + pair means, then gradients + loss scalars.
template <bool GROUPED>
static int launch_nce_selected(const float* S, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld, int softplus,
                               float reg, const int* groups, int mode, int n_neg, unsigned long long seed, unsigned long long draw,
                               int dtype, hipStream_t stream) {
    unsigned long long* thr = (unsigned long long*)workspace;
    float* lse = workspace + 2LL * K * B;
    float* pairp = lse + (long long)K * B;
    const int nmb = (int)(((long long)B * B + 255) / 256);
    float* mean = pairp + 3LL * nmb;
    const int ncb = (K * B + NSM_COLS - 1) / NSM_COLS;
    const int nb = (ld + 31) / 32;
    const dim3 g1(ncb + nmb);
#define NSM_COL(KT, H) \
    hipLaunchKernelGGL((nce_selected_col_mean_kernel<GROUPED, KT, H>), g1, dim3(256), 0, stream, S, thr, lse, mean, pairp, B, K, ld, softplus, \
                       groups, mode, n_neg, seed, draw, ncb)
    if (B <= 256) {
        if (K == 12) NSM_COL(12, 4); else if (K == 16) NSM_COL(16, 4); else NSM_COL(0, 4);
    } else {
        if (K == 12) NSM_COL(12, 16); else if (K == 16) NSM_COL(16, 16); else NSM_COL(0, 16);
    }
#undef NSM_COL
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((nce_selected_grad_kernel<bf16_t, GROUPED>), dim3(nb, nb, K), dim3(256), 0, stream, S, lse, thr, mean, (bf16_t*)dS,
                           (bf16_t*)dST, B, K, ld, softplus, reg, groups, mode, seed, draw, pairp, nmb, out);
    else
        hipLaunchKernelGGL((nce_selected_grad_kernel<float, GROUPED>), dim3(nb, nb, K), dim3(256), 0, stream, S, lse, thr, mean, (float*)dS,
                           (float*)dST, B, K, ld, softplus, reg, groups, mode, seed, draw, pairp, nmb, out);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

template <bool GROUPED>
static int launch_nce_select_mask(unsigned char* mask, const int* groups, int B, int K, int mode, int n_neg, unsigned long long seed,
                                  unsigned long long draw, hipStream_t stream) {
    const dim3 grid((K * B + NSM_COLS - 1) / NSM_COLS);
    if (B <= 256) hipLaunchKernelGGL((nce_select_mask_kernel<GROUPED, 4>), grid, dim3(256), 0, stream, mask, groups, B, K, mode, n_neg, seed, draw);
    else hipLaunchKernelGGL((nce_select_mask_kernel<GROUPED, 16>), grid, dim3(256), 0, stream, mask, groups, B, K, mode, n_neg, seed, draw);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// (the dtype and the alignment are checked before the first launch: a refused call writes nothing)
int launch_nce_sampled(const float* S, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld, int softplus, float reg,
                       int n_neg, unsigned long long seed, unsigned long long draw, int dtype, hipStream_t stream) {
    if (B <= 1 || B > NSM_MAXB || K <= 0 || ld < B || ld > B + 7 || n_neg < 1 || n_neg > B - 1) return CPC_EINVAL;
    if ((dtype != CPC_DTYPE_BF16 && dtype != CPC_DTYPE_F32) || (uintptr_t)workspace % 8) return CPC_EINVAL;
    return launch_nce_selected<false>(S, dS, dST, out, workspace, B, K, ld, softplus, reg, nullptr, 0, n_neg, seed, draw, dtype, stream);
}

int launch_nce_sample_mask(unsigned char* mask, int B, int K, int n_neg, unsigned long long seed, unsigned long long draw,
                           hipStream_t stream) {
    if (!mask || B <= 1 || B > NSM_MAXB || K <= 0 || n_neg < 1 || n_neg > B - 1) return CPC_EINVAL;
    return launch_nce_select_mask<false>(mask, nullptr, B, K, 0, n_neg, seed, draw, stream);
}

int launch_nce_grouped(const float* S, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld, int softplus, float reg,
                       const int* groups, int mode, int n_neg, unsigned long long seed, unsigned long long draw, int dtype,
                       hipStream_t stream) {
    if (!groups || B <= 1 || B > NSM_MAXB || K <= 0 || ld < B || ld > B + 7 || n_neg < 0 || n_neg > B - 1 || (mode != 0 && mode != 1)) return CPC_EINVAL;
    if ((dtype != CPC_DTYPE_BF16 && dtype != CPC_DTYPE_F32) || (uintptr_t)workspace % 8) return CPC_EINVAL;
    return launch_nce_selected<true>(S, dS, dST, out, workspace, B, K, ld, softplus, reg, groups, mode, n_neg, seed, draw, dtype, stream);
}

int launch_nce_group_mask(unsigned char* mask, const int* groups, int B, int K, int mode, int n_neg, unsigned long long seed,
                          unsigned long long draw, hipStream_t stream) {
    if (!mask || !groups || B <= 1 || B > NSM_MAXB || K <= 0 || n_neg < 0 || n_neg > B - 1 || (mode != 0 && mode != 1)) return CPC_EINVAL;
    return launch_nce_select_mask<true>(mask, groups, B, K, mode, n_neg, seed, draw, stream);
}

// ---- negative bank ----
// workspace: chunk pairs (max, sum) [slots * ceil(B / NBK_CHUNK)][K][B] (8 bytes each, first: the workspace must be 8-byte aligned)
// + lse [K][B] + column partials [ceil(K B / 256)] + pair partials [3 * ceil(B*B/256)] + pair means [B][ld <= B + 7]
long long nce_banked_workspace_floats(int B, int K, int slots) {
    if (B <= 0 || K <= 0 || slots <= 0) return 0;
    const long long nmb = ((long long)B * B + 255) / 256, cps = (B + NBK_CHUNK - 1) / NBK_CHUNK;
    return 2LL * slots * cps * K * B + (long long)K * B + ((long long)K * B + 255) / 256 + 3 * nmb + (long long)B * (B + 8);
}

// (K <= NBK_MAXK keeps K B, the chunk count and every grid dimension far inside an int; one CPC_CHECK_LAUNCH behind the last launch,
// as the siblings: a launch that fails leaves its error for it)
constexpr int NBK_MAXK = 1024;

int launch_nce_banked(const float* S, void* dS, void* dST_cur, float* out, float* workspace, int B, int K, int ld, int slots, int cur,
                      unsigned long long valid, int softplus, float reg, int dtype, hipStream_t stream) {
    if (B <= 1 || B > NSM_MAXB || K <= 0 || K > NBK_MAXK || ld < B || ld > B + 7 || slots < 2 || slots > 64 || cur < 0 || cur >= slots) return CPC_EINVAL;
    if (!nbk_valid(valid, cur) || (slots < 64 && (valid >> slots) != 0)) return CPC_EINVAL;
    if ((dtype != CPC_DTYPE_BF16 && dtype != CPC_DTYPE_F32) || (uintptr_t)workspace % 8) return CPC_EINVAL;
    const int cps = (B + NBK_CHUNK - 1) / NBK_CHUNK, nchunk = slots * cps;
    const int nmb = (int)(((long long)B * B + 255) / 256), ncolp = (K * B + 255) / 256;
    float2* part = (float2*)workspace;
    float* lse = workspace + 2LL * nchunk * K * B;
    float* colp = lse + (long long)K * B;
    float* pairp = colp + ncolp;
    float* mean = pairp + 3LL * nmb;
    const int ncb = (B + 63) / 64;
    const int npart = K * ((nchunk + NBK_WAVES - 1) / NBK_WAVES) * ncb;
    const dim3 g1(npart + nmb);
#define NBK_PART(KT) \
    hipLaunchKernelGGL(nce_bank_partial_mean_kernel<KT>, g1, dim3(256), 0, stream, S, part, mean, pairp, B, K, ld, slots, cur, valid, softplus, \
                       cps, ncb, npart)
    if (K == 12) NBK_PART(12); else if (K == 16) NBK_PART(16); else NBK_PART(0);
#undef NBK_PART
    hipLaunchKernelGGL(nce_bank_merge_kernel, dim3(ncolp), dim3(256), 0, stream, part, nchunk, cps, valid, K * B, lse, colp);
    const dim3 g3((ld + 31) / 32, slots * ((ld + 31) / 32), K);
    if (dtype == CPC_DTYPE_BF16)
        hipLaunchKernelGGL((nce_bank_grad_kernel<bf16_t>), g3, dim3(256), 0, stream, S, lse, mean, (bf16_t*)dS, (bf16_t*)dST_cur, B, K, ld,
                           slots, cur, valid, softplus, reg, colp, ncolp, pairp, nmb, out);
    else
        hipLaunchKernelGGL((nce_bank_grad_kernel<float>), g3, dim3(256), 0, stream, S, lse, mean, (float*)dS, (float*)dST_cur, B, K, ld,
                           slots, cur, valid, softplus, reg, colp, ncolp, pairp, nmb, out);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// ---- score_over_all_timesteps = True ----
static const int NCE_ALL_BLOCKS = 3072;
static const int NCE_ALL_SPLITS = 16;
// workspace: lse [R] + col partials [ceil(R/32)] + grad partials [3 * NCE_ALL_BLOCKS] + per-split (max, sum) [2][NCE_ALL_SPLITS][R]
long long nce_all_workspace_floats(int B, int K) {
    const long long R = (long long)B * K;
    return R + (R + 31) / 32 + 3LL * NCE_ALL_BLOCKS + 2LL * NCE_ALL_SPLITS * R;
}

int launch_nce_all(const float* S, const float* ST, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld,
                   int softplus, float reg, int dtype, hipStream_t stream) {
    const int R = B * K;
    if (B <= 0 || K <= 0 || ld < R) return CPC_EINVAL;
    if (dtype != CPC_DTYPE_BF16 && dtype != CPC_DTYPE_F32) return CPC_EINVAL;       // before the first launch: a refused call writes nothing
    float* lse = workspace;
    const int ncb = (R + 31) / 32;
    float* colp = lse + R;
    float* gradp = colp + ncb;
    float* pm = gradp + 3LL * NCE_ALL_BLOCKS;
    float* ps = pm + (long long)NCE_ALL_SPLITS * R;
    const int nsplit = R >= 8 * NCE_ALL_SPLITS ? NCE_ALL_SPLITS : 1;
    int n_colp = ncb;
    if (nsplit > 1) {
        const int rps = ((R + nsplit - 1) / nsplit + 7) / 8 * 8;
        hipLaunchKernelGGL(nce_col_kernel, dim3(ncb, 1, nsplit), dim3(256), 0, stream, S, lse, colp, R, 1, ld, softplus, rps, pm, ps);
        n_colp = (R + 255) / 256;
        hipLaunchKernelGGL(nce_col_merge_kernel, dim3(n_colp), dim3(256), 0, stream, pm, ps, nsplit, R, lse, colp);
    } else {
        hipLaunchKernelGGL(nce_col_kernel, dim3(ncb, 1, 1), dim3(256), 0, stream, S, lse, colp, R, 1, ld, softplus, R, (float*)nullptr,
                           (float*)nullptr);
    }
    const long long total = (long long)B * R;
    const int blocks = (int)min((long long)NCE_ALL_BLOCKS, (total + 255) / 256);
#define NCE_ALL_GRAD(T, KT) \
    do { \
        hipLaunchKernelGGL((nce_all_grad_kernel<T, true, KT>), dim3(blocks), dim3(256), 0, stream, S, lse, (T*)dS, gradp, B, K, 1LL, \
                           (long long)ld, softplus, reg, 1); \
        hipLaunchKernelGGL((nce_all_grad_kernel<T, false, KT>), dim3(blocks), dim3(256), 0, stream, ST, lse, (T*)dST, gradp, B, K, \
                           (long long)ld, 1LL, softplus, reg, 0); \
    } while (0)
    if (dtype == CPC_DTYPE_BF16) {
        if (K == 12) NCE_ALL_GRAD(bf16_t, 12); else if (K == 16) NCE_ALL_GRAD(bf16_t, 16); else NCE_ALL_GRAD(bf16_t, 0);
    } else {
        if (K == 12) NCE_ALL_GRAD(float, 12); else if (K == 16) NCE_ALL_GRAD(float, 16); else NCE_ALL_GRAD(float, 0);
    }
#undef NCE_ALL_GRAD
    hipLaunchKernelGGL(nce_all_finalize_kernel, dim3(1), dim3(256), 0, stream, colp, n_colp, gradp, blocks, out, B, K, reg);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}


// ---- validation ----
// workspace: lse [R] + column partials + per-split (max, sum) [2][NCE_ALL_SPLITS][R] + row sums / arg max / valid [3][R]   (R = B*K)
long long nce_eval_workspace_floats(int B, int K) {
    const long long R = (long long)B * K;
    return R + (R + 31) / 32 + K * (long long)((B + 31) / 32) + 2LL * NCE_ALL_SPLITS * R + 3 * R + 64;
}

int launch_nce_eval(const float* S, float* out, float* workspace, int B, int K, int ld, int softplus, int all_timesteps,
                    int accumulate, hipStream_t stream) {
    const int R = B * K;
    if (B <= 0 || K <= 0 || (all_timesteps ? ld < R : (ld < B || ld > B + 7))) return CPC_EINVAL;
    float* lse = workspace;
    float* colp = lse + R;
    float* pm = colp + (R + 31) / 32 + (long long)K * ((B + 31) / 32);
    float* ps = pm + (long long)NCE_ALL_SPLITS * R;
    float* rsum = ps + (long long)NCE_ALL_SPLITS * R;
    int* rarg = (int*)(rsum + R);
    float* rvalid = rsum + 2LL * R;
    if (all_timesteps) {
        const int ncb = (R + 31) / 32;
        const int nsplit = R >= 8 * NCE_ALL_SPLITS ? NCE_ALL_SPLITS : 1;
        if (nsplit > 1) {
            const int rps = ((R + nsplit - 1) / nsplit + 7) / 8 * 8;
            hipLaunchKernelGGL(nce_col_kernel, dim3(ncb, 1, nsplit), dim3(256), 0, stream, S, lse, colp, R, 1, ld, softplus, rps, pm, ps);
            hipLaunchKernelGGL(nce_col_merge_kernel, dim3((R + 255) / 256), dim3(256), 0, stream, pm, ps, nsplit, R, lse, colp);
        } else {
            hipLaunchKernelGGL(nce_col_kernel, dim3(ncb, 1, 1), dim3(256), 0, stream, S, lse, colp, R, 1, ld, softplus, R, (float*)nullptr,
                               (float*)nullptr);
        }
        hipLaunchKernelGGL(nce_row_eval_kernel, dim3((R + 3) / 4), dim3(256), 0, stream, S, R, R, ld, 0, softplus, rsum, rarg, rvalid);
    } else {
        hipLaunchKernelGGL(nce_col_kernel, dim3((B + 31) / 32, K, 1), dim3(256), 0, stream, S, lse, colp, B, K, ld, softplus, B,
                           (float*)nullptr, (float*)nullptr);
        hipLaunchKernelGGL(nce_row_eval_kernel, dim3((R + 3) / 4), dim3(256), 0, stream, S, R, B, ld, B, softplus, rsum, rarg, rvalid);
    }
    hipLaunchKernelGGL(nce_eval_finalize_kernel, dim3(1), dim3(256), 0, stream, lse, rsum, rarg, rvalid, out, B, K, all_timesteps ? 1 : 0,
                       accumulate ? 1 : 0);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// Wasserstein gradient penalty with softplus scores (contrastive_estimation_training.py:12-16 under :144-158): the summed scores
// are sum softplus(s), so the seeds of the penalty's passes carry the coefficients sigmoid(s) (first order) and
// sigmoid'(s) * (tangent of s) (second order) instead of the constant 1 and 0 of linear scores.
//   mode 0:  w = d softplus(s) / d s          mode 1:  w = d^2 softplus(s) / d s^2 * (St1 + St2)     (St2 may be NULL)
// S, St*: nmat matrices [rows][ld] f32;  W [nmat][rows][ld], WT [nmat][cols][ldT] (the transpose), both f32.
__global__ __launch_bounds__(256) void gp_score_coeff_kernel(const float* __restrict__ S, const float* __restrict__ St1,
                                                             const float* __restrict__ St2, float* __restrict__ W,
                                                             float* __restrict__ WT, int rows, int cols, int ld, int ldT, int mode) {
    const int m = blockIdx.y;
    const long long total = (long long)rows * cols;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int r = (int)(idx / cols), c = (int)(idx % cols);
        const long long o = ((long long)m * rows + r) * ld + c;
        const float x = S[o];
        const float sg = x > 20.f ? 1.f : 1.f / (1.f + expf(-x));
        float w = sg;
        if (mode == 1) {
            float t = St1[o];
            if (St2) t += St2[o];
            w = x > 20.f ? 0.f : sg * (1.f - sg) * t;
        }
        W[o] = w;
        WT[((long long)m * cols + c) * ldT + r] = w;
    }
}

int launch_gp_score_coeff(const float* S, const float* St1, const float* St2, float* W, float* WT, int nmat, int rows, int cols, int ld,
                          int ldT, int mode, hipStream_t stream) {
    if (nmat <= 0 || rows <= 0 || cols <= 0 || ld < cols || ldT < rows || (mode != 0 && mode != 1) || (mode == 1 && !St1)) return CPC_EINVAL;
    const int blocks = (int)std::min<long long>(1024, ((long long)rows * cols + 255) / 256);
    hipLaunchKernelGGL(gp_score_coeff_kernel, dim3(blocks, nmat), dim3(256), 0, stream, S, St1, St2, W, WT, rows, cols, ld, ldT, mode);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
