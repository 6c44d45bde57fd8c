// ABX discriminability (include/cpc_hip.h, cpc_frame_distance / cpc_dtw / cpc_abx_count; DESIGN.md, "ABX discriminability").
//   frame distances  a wave forms the distances of up to 64 rows of segment A against up to 32 rows of segment B: the A rows are the
//                    MFMA's row operand (two 32 x 32 tiles), the B rows its column operand, read from the feature store 4 columns per
//                    lane and step (lane half h takes columns 8 s + 4 h .. + 3 of step s); the products are f32-input MFMAs (32x32x2:
//                    an fmaf chain, one rounding per product, the column order fixed by D alone).  The squared norms come from the very
//                    operand registers (per lane half an fmaf chain over its columns, the two halves added once).  dtw_block is the ONE
//                    place that forms a distance: cpc_frame_distance writes what it leaves in LDS, cpc_dtw sweeps it.
//   dtw              one wave per pair.  Lane i owns row i of a stripe of 64 rows and sweeps the anti-diagonals of a block of 32 columns:
//                    its left neighbour is its own previous value, its upper neighbour lane i - 1's previous value (one cross-lane shift
//                    of (C, len) per step) and its diagonal neighbour what it received one step earlier.  Values persist across the
//                    column blocks of a stripe; the last row of the first stripe is kept in LDS for the second.  The La x Lb distances
//                    and costs never reach HBM.
//   abx count        one workgroup per (cell, p, q) task: per column x the two distance columns go through LDS, the comparisons are
//                    integer counts folded by a fixed tree.
#include <cmath>
#include "cpc_common.h"
#include "cpc_kernels.h"
#include "../../include/cpc_hip.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int DT_ROWS = 64;              // rows of a stripe: one per lane
constexpr int DT_COLS = 32;              // columns of a block: one MFMA tile
constexpr int DT_LD = 40;                // LDS row stride in floats: the sweep reads (i, t - i), 39 i + t: 32 banks once per 32 lanes
constexpr int DT_MAXLEN = 128;
constexpr float DT_NORM_MAX = 0x1p116f;  // the largest squared norm of a row that counts as finite: 4 * 256 * 2^116 < FLT_MAX

__device__ __forceinline__ unsigned dt_nonfinite_bit(float v) {
    return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
}

// The frame distance from the dot product and the two squared norms.  No product feeds a sum outside an explicit fmaf, so the compiler
// has nothing to contract differently in the two kernels.
__device__ __forceinline__ float dt_distance(float dot, float na2, float nb2, int metric) {
    if (metric == 2) return fmaxf(fmaf(-2.f, dot, na2 + nb2), 0.f);
    const float c = fminf(fmaxf(dot / (sqrtf(na2) * sqrtf(nb2)), -1.f), 1.f);
    if (metric == 1) return 1.f - c;
    return acosf(c) / 3.14159274f;
}

// Distances of rows [arow0, + na) against rows [brow0, + nb) of x (1 <= na <= 64, 1 <= nb <= 32; all of them rows of the store) into
// ds[i * DT_LD + j]; an_s: 64 floats.  Lanes beyond na / nb work on the last valid row, so every address is one of a valid row and
// the cells they fill are never read.  Returns this lane's share of "a row holds a NaN or an infinity, has a squared norm above
// DT_NORM_MAX, or (metrics 0, 1) has the norm 0".
// The caller synchronises before the call (ds and an_s may still be read) and after it.
template <typename T>
__device__ __forceinline__ unsigned dtw_block(const T* __restrict__ x, long long ldx, int D, long long arow0, int na, long long brow0,
                                              int nb, int metric, float* ds, float* an_s) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const bool two = na > 32;
    const T* pa0 = x + (arow0 + min(j, na - 1)) * ldx + 4 * h;
    const T* pa1 = x + (arow0 + min(32 + j, na - 1)) * ldx + 4 * h;
    const T* pb = x + (brow0 + min(j, nb - 1)) * ldx + 4 * h;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    float sa0 = 0.f, sa1 = 0.f, sb = 0.f;
    unsigned bad = 0u;
    const int ns = D >> 3;
    f32x4 a0 = load4(pa0), b = load4(pb), a1 = two ? load4(pa1) : a0;
    for (int s = 0; s < ns; ++s) {
        const int nxt = min(s + 1, ns - 1) * 8;                  // (the last step reloads itself: no read past the row)
        const f32x4 a0n = load4(pa0 + nxt), bn = load4(pb + nxt), a1n = two ? load4(pa1 + nxt) : a0n;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b[e], acc0, 0, 0, 0);
            sa0 = fmaf(a0[e], a0[e], sa0);
            sb = fmaf(b[e], b[e], sb);
            bad |= dt_nonfinite_bit(a0[e]) | dt_nonfinite_bit(b[e]);
        }
        if (two) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], b[e], acc1, 0, 0, 0);
                sa1 = fmaf(a1[e], a1[e], sa1);
                bad |= dt_nonfinite_bit(a1[e]);
            }
        }
        a0 = a0n; a1 = a1n; b = bn;
    }
    // the two lane halves of a row hold the two halves of its columns
    sa0 += __shfl_xor(sa0, 32);
    sa1 += __shfl_xor(sa1, 32);
    sb += __shfl_xor(sb, 32);
    if (metric != 2) bad |= (sa0 == 0.f || sb == 0.f || (two && sa1 == 0.f)) ? 1u : 0u;
    // finite rows whose squared norm is not: with the norms at most DT_NORM_MAX every distance (at most 4 of them) and every sum along
    // a path of 255 cells stays finite, so that +inf can stand for a neighbour that does not exist (!(v <= max) also catches a NaN)
    bad |= (!(sa0 <= DT_NORM_MAX) || !(sb <= DT_NORM_MAX) || (two && !(sa1 <= DT_NORM_MAX))) ? 1u : 0u;
    an_s[lane] = h ? sa1 : sa0;                                   // lane 32 + j: row 32 + j of the stripe
    __syncthreads();
    // accumulator register r: row (r & 3) + 8 (r >> 2) + 4 h of the tile against column j
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 n0 = *(const f32x4*)(an_s + 8 * q + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) ds[(8 * q + 4 * h + e) * DT_LD + j] = dt_distance(acc0[4 * q + e], n0[e], sb, metric);
    }
    if (two) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 n1 = *(const f32x4*)(an_s + 32 + 8 * q + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) ds[(32 + 8 * q + 4 * h + e) * DT_LD + j] = dt_distance(acc1[4 * q + e], n1[e], sb, metric);
        }
    }
    return bad;
}

// ------------------------------------------------------------------------------------------------------------ frame distance
// Workgroup (bx, by), one wave: rows [64 by, + 64) of segment A against rows [32 bx, + 32) of segment B.
template <typename T>
__global__ __launch_bounds__(64) void frame_distance_kernel(const T* __restrict__ x, int D, long long ldx, long long a_first, int La,
                                                            long long b_first, int Lb, int metric, float* __restrict__ out,
                                                            long long ldo) {
    __shared__ __attribute__((aligned(16))) float ds[DT_ROWS * DT_LD];
    __shared__ __attribute__((aligned(16))) float an_s[DT_ROWS];
    const int lane = threadIdx.x, i0 = DT_ROWS * blockIdx.y, j0 = DT_COLS * blockIdx.x;
    const int na = min(DT_ROWS, La - i0), nb = min(DT_COLS, Lb - j0);
    dtw_block<T>(x, ldx, D, a_first + i0, na, b_first + j0, nb, metric, ds, an_s);
    __syncthreads();
    const int j = lane & 31;
    if (j < nb)
        for (int i = lane >> 5; i < na; i += 2) out[(long long)(i0 + i) * ldo + j0 + j] = ds[i * DT_LD + j];
}

// ----------------------------------------------------------------------------------------------------------------------- dtw
template <typename T>
__global__ __launch_bounds__(64) void dtw_kernel(const T* __restrict__ x, long long N, int D, long long ldx,
                                                 const long long* __restrict__ pairs, int metric, float* __restrict__ dist,
                                                 float* __restrict__ cost, int* __restrict__ path_len) {
    __shared__ __attribute__((aligned(16))) float ds[DT_ROWS * DT_LD];
    __shared__ __attribute__((aligned(16))) float an_s[DT_ROWS];
    __shared__ float carry_c[DT_MAXLEN];
    __shared__ int carry_l[DT_MAXLEN];
    const int lane = threadIdx.x;
    const long long p = blockIdx.x;
    const long long a_first = pairs[4 * p], la = pairs[4 * p + 1], b_first = pairs[4 * p + 2], lb = pairs[4 * p + 3];
    // a table row out of range: the NaN result, and no address formed from it (uniform over the wave, which is the workgroup)
    const bool ok = la >= 1 && la <= DT_MAXLEN && lb >= 1 && lb <= DT_MAXLEN && a_first >= 0 && a_first <= N - la && b_first >= 0 &&
                    b_first <= N - lb;
    float res_c = NAN;
    int res_l = -1;
    if (ok) {
        const int La = (int)la, Lb = (int)lb;
        unsigned bad = 0u;
        float cur_c = INFINITY;
        int cur_l = 0;
        for (int i0 = 0; i0 < La; i0 += DT_ROWS) {
            const int na = min(DT_ROWS, La - i0);
            cur_c = INFINITY;                      // (left of column 0: nothing)
            cur_l = 0;
            float pu_c = INFINITY;                 // lane i - 1's value one step earlier: the diagonal neighbour
            int pu_l = 0;
            for (int j0 = 0; j0 < Lb; j0 += DT_COLS) {
                const int nb = min(DT_COLS, Lb - j0);
                __syncthreads();
                bad |= dtw_block<T>(x, ldx, D, a_first + i0, na, b_first + j0, nb, metric, ds, an_s);
                __syncthreads();
                const float* drow = ds + lane * DT_LD;
                for (int t = 0; t < na + nb - 1; ++t) {
                    float u_c = __shfl_up(cur_c, 1);
                    int u_l = __shfl_up(cur_l, 1);
                    const int jj = t - lane;
                    if (lane < na && jj >= 0 && jj < nb) {
                        const int jg = j0 + jj;
                        if (lane == 0) {           // the row above the stripe: nothing, or the last row of the first stripe
                            if (i0 == 0) {
                                u_c = INFINITY;
                                pu_c = jg == 0 ? 0.f : INFINITY;          // (the start cell: a path of no cells before it)
                                u_l = pu_l = 0;
                            } else {
                                u_c = carry_c[jg];
                                u_l = carry_l[jg];
                                pu_c = jg > 0 ? carry_c[jg - 1] : INFINITY;
                                pu_l = jg > 0 ? carry_l[jg - 1] : 0;
                            }
                        }
                        const float d = drow[jj];
                        float m;
                        int l;
                        if (pu_c <= u_c && pu_c <= cur_c) { m = pu_c; l = pu_l; }          // the diagonal, then the left, then the upper
                        else if (cur_c <= u_c) { m = cur_c; l = cur_l; }
                        else { m = u_c; l = u_l; }
                        cur_c = d + m;
                        cur_l = l + 1;
                        if (lane == DT_ROWS - 1 && i0 == 0 && La > DT_ROWS) {          // what the second stripe's first row needs
                            carry_c[jg] = cur_c;
                            carry_l[jg] = cur_l;
                        }
                    }
                    pu_c = u_c;
                    pu_l = u_l;
                }
            }
        }
        const int last = (La - 1) & (DT_ROWS - 1);
        const float end_c = __shfl(cur_c, last);
        const int end_l = __shfl(cur_l, last);
        if (!__any(bad != 0u)) { res_c = end_c; res_l = end_l; }
    }
    if (lane == 0) {
        dist[p] = res_l > 0 ? res_c / (float)res_l : NAN;
        if (cost) cost[p] = res_c;
        if (path_len) path_len[p] = res_l;
    }
}

// ----------------------------------------------------------------------------------------------------------------- abx count
// Task t = blockIdx.x.  Per column x of group p: the distances of the items of p and of q to x go through LDS; thread a-strided
// counts 2 [d(a, x) < d(b, x)] + [d(a, x) == d(b, x)] over b for its a != x.
__global__ __launch_bounds__(256) void abx_count_kernel(const float* __restrict__ dist, long long n_dist, const long long* __restrict__ tasks,
                                                        long long* __restrict__ out) {
    __shared__ float ap[1024], bq[1024];
    __shared__ long long red[256];
    __shared__ int nan_s[256];
    const int t = threadIdx.x;
    const long long* q = tasks + 6 * (long long)blockIdx.x;
    const long long off = q[0], nc = q[1], sp = q[2], np = q[3], sq = q[4], nq = q[5];
    const bool ok = np >= 2 && np <= 1024 && nq >= 1 && nq <= 1024 && nc >= 1 && nc <= 0x7FFFFFFFll && sp >= 0 && sp <= nc - np &&
                    sq >= 0 && sq <= nc - nq && off >= 0 && nc * nc <= n_dist && off <= n_dist - nc * nc;
    if (!ok) {
        if (t == 0) out[blockIdx.x] = -2;
        return;
    }
    const float* cell = dist + off;
    long long cnt = 0;
    int sawnan = 0;
    for (int xi = 0; xi < (int)np; ++xi) {
        __syncthreads();
        for (int i = t; i < (int)np; i += 256) {
            const float v = i == xi ? 0.f : cell[(sp + i) * nc + sp + xi];          // d(x, x) is never read
            sawnan |= v != v;
            ap[i] = v;
        }
        for (int i = t; i < (int)nq; i += 256) {
            const float v = cell[(sq + i) * nc + sp + xi];
            sawnan |= v != v;
            bq[i] = v;
        }
        __syncthreads();
        for (int a = t; a < (int)np; a += 256) {
            if (a == xi) continue;
            const float da = ap[a];
            int c = 0;
            for (int b = 0; b < (int)nq; ++b) {
                const float db = bq[b];
                c += (da < db ? 2 : 0) + (da == db ? 1 : 0);
            }
            cnt += c;
        }
    }
    red[t] = cnt;
    nan_s[t] = sawnan;
#pragma unroll
    for (int m = 128; m > 0; m >>= 1) {
        __syncthreads();
        if (t < m) {
            red[t] += red[t + m];
            nan_s[t] |= nan_s[t + m];
        }
    }
    if (t == 0) out[blockIdx.x] = nan_s[0] ? -1 : red[0];
}

}  // namespace

int launch_frame_distance(const void* x, int dtype, int D, long long ldx, long long a_first, int La, long long b_first, int Lb, int metric,
                          float* out, long long ldo, hipStream_t stream) {
    const dim3 grid((unsigned)((Lb + DT_COLS - 1) / DT_COLS), (unsigned)((La + DT_ROWS - 1) / DT_ROWS));
    if (dtype == CPC_DTYPE_BF16)
        frame_distance_kernel<bf16_t><<<grid, 64, 0, stream>>>((const bf16_t*)x, D, ldx, a_first, La, b_first, Lb, metric, out, ldo);
    else
        frame_distance_kernel<float><<<grid, 64, 0, stream>>>((const float*)x, D, ldx, a_first, La, b_first, Lb, metric, out, ldo);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// The HIP runtime refuses a launch whose gridDim.x * blockDim.x reaches 2^32, so a table goes out in grids of at most 2^31 threads:
// 2^25 pairs of one wave, 2^23 tasks of four.  Each grid gets its part of the table and of the outputs as its base pointers.
constexpr long long DT_GRID_PAIRS = (1ll << 31) / 64;
constexpr long long DT_GRID_TASKS = (1ll << 31) / 256;

int launch_dtw(const void* x, int dtype, long long N, int D, long long ldx, const long long* pairs, long long P, int metric, float* dist,
               float* cost, int* path_len, hipStream_t stream) {
    for (long long p0 = 0; p0 < P; p0 += DT_GRID_PAIRS) {
        const unsigned grid = (unsigned)(P - p0 < DT_GRID_PAIRS ? P - p0 : DT_GRID_PAIRS);
        float* c = cost ? cost + p0 : nullptr;
        int* l = path_len ? path_len + p0 : nullptr;
        if (dtype == CPC_DTYPE_BF16)
            dtw_kernel<bf16_t><<<grid, 64, 0, stream>>>((const bf16_t*)x, N, D, ldx, pairs + 4 * p0, metric, dist + p0, c, l);
        else
            dtw_kernel<float><<<grid, 64, 0, stream>>>((const float*)x, N, D, ldx, pairs + 4 * p0, metric, dist + p0, c, l);
        CPC_CHECK_LAUNCH();
    }
    return CPC_OK;
}

int launch_abx_count(const float* dist, long long n_dist, const long long* tasks, long long T, long long* out, hipStream_t stream) {
    for (long long t0 = 0; t0 < T; t0 += DT_GRID_TASKS) {
        const unsigned grid = (unsigned)(T - t0 < DT_GRID_TASKS ? T - t0 : DT_GRID_TASKS);
        abx_count_kernel<<<grid, 256, 0, stream>>>(dist, n_dist, tasks + 6 * t0, out + t0);
        CPC_CHECK_LAUNCH();
    }
    return CPC_OK;
}
