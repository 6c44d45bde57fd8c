// Difference scores (contrastive_estimation_training.py:25-33, difference_score_function): s[r][c] = 1 / sum_e (p[r][e] - t[c][e])^2,
// formed as differences (never through |p|^2 + |t|^2 - 2 p.t, which cancels exactly where the score is largest), and the
// element-wise part of their backward.  VALU work: f32 sub + fma, packed two columns per instruction (v_pk_add_f32 / v_pk_fma_f32).
#include "cpc_common.h"
#include "cpc_kernels.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int DS_TILE = 64;        // 64 x 64 outputs per workgroup, 4 x 4 per lane
constexpr int DS_EK = 32;          // feature chunk staged in LDS per pass
constexpr int DS_PAD = 4;          // LDS row padding (floats): keeps the 16-byte reads aligned, spreads the transposing writes

// Loads 8 consecutive features [e0, e0 + 8) of one row as f32 (zeros past E or for a row outside the matrix).
template <typename T, bool VEC>
__device__ __forceinline__ void load8(const T* row, int e0, int E, bool valid, float (&v)[8]) {
    if (VEC) {
        // E % 8 == 0 (bf16) / E % 4 == 0 (f32) and 16-byte aligned rows: a 4-element half is wholly inside or outside [0, E)
        for (int h = 0; h < 2; ++h) {
            const int e = e0 + 4 * h;
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (valid && e < E) x = load4(row + e);
            v[4 * h + 0] = x[0]; v[4 * h + 1] = x[1]; v[4 * h + 2] = x[2]; v[4 * h + 3] = x[3];
        }
    } else {
        for (int q = 0; q < 8; ++q) v[q] = (valid && e0 + q < E) ? to_f32(row[e0 + q]) : 0.f;
    }
}

// S[z][m][n] = 1 / sum_e (P[z][m][e] - T[z][n][e])^2 and, when ST != NULL, ST[z][n][m] = the same value.
// P row m of batch z at z * p_batch + m * ldp; T row n at z * t_batch + row_off(n, t_rpi, t_item, ldt); S / ST rows of lds floats.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void diff_scores_kernel(const T* __restrict__ P, const T* __restrict__ Tg, float* __restrict__ S,
                                                          float* __restrict__ ST, int M, int N, int E, long long ldp, long long ldt,
                                                          int t_rpi, long long t_item, long long p_batch, long long t_batch,
                                                          long long s_batch, int lds) {
    __shared__ __attribute__((aligned(16))) float sP[DS_EK][DS_TILE + DS_PAD];
    __shared__ __attribute__((aligned(16))) float sT[DS_EK][DS_TILE + DS_PAD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * DS_TILE, n0 = blockIdx.x * DS_TILE, z = blockIdx.z;
    P += z * p_batch;
    Tg += z * t_batch;

    // staging: lane tid loads features [8 (tid & 3), +8) of tile row tid >> 2 of both operands
    const int lr = tid >> 2, le = (tid & 3) * 8;
    const bool pv = m0 + lr < M, tv = n0 + lr < N;
    const T* prow = P + (pv ? (long long)(m0 + lr) * ldp : 0);
    const T* trow = Tg + (tv ? row_off(n0 + lr, t_rpi, t_item, ldt) : 0);

    f32x2 acc[4][2];
    for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = f32x2{0.f, 0.f};

    for (int e0 = 0; e0 < E; e0 += DS_EK) {
        float vp[8], vt[8];
        load8<T, VEC>(prow, e0 + le, E, pv, vp);
        load8<T, VEC>(trow, e0 + le, E, tv, vt);
        __syncthreads();                    // the previous chunk's reads are done
        for (int q = 0; q < 8; ++q) {
            sP[le + q][lr] = vp[q];
            sT[le + q][lr] = vt[q];
        }
        __syncthreads();
#pragma unroll 8
        for (int e = 0; e < DS_EK; ++e) {
            const f32x4 a = *(const f32x4*)&sP[e][ty * 4];
            const f32x4 b = *(const f32x4*)&sT[e][tx * 4];
            const f32x2 b01 = {b[0], b[1]}, b23 = {b[2], b[3]};
            for (int i = 0; i < 4; ++i) {
                const f32x2 ai = {a[i], a[i]};
                const f32x2 d0 = ai - b01, d1 = ai - b23;
                acc[i][0] = __builtin_elementwise_fma(d0, d0, acc[i][0]);
                acc[i][1] = __builtin_elementwise_fma(d1, d1, acc[i][1]);
            }
        }
    }

    float s[4][4];
    for (int i = 0; i < 4; ++i) {
        s[i][0] = 1.0f / acc[i][0][0]; s[i][1] = 1.0f / acc[i][0][1];
        s[i][2] = 1.0f / acc[i][1][0]; s[i][3] = 1.0f / acc[i][1][1];
    }
    const int mb = m0 + ty * 4, nb = n0 + tx * 4;
    float* Sz = S + z * s_batch;
    // lds % 4 == 0 and S 16-byte aligned (checked by the launcher when VEC): whole 4-float rows of the block are one store
    for (int i = 0; i < 4; ++i) {
        const int m = mb + i;
        if (m >= M) break;
        float* o = Sz + (long long)m * lds + nb;
        if (VEC && nb + 3 < N) {
            *(f32x4*)o = f32x4{s[i][0], s[i][1], s[i][2], s[i][3]};
        } else {
            for (int j = 0; j < 4; ++j)
                if (nb + j < N) o[j] = s[i][j];
        }
    }
    if (ST == nullptr) return;
    float* STz = ST + z * s_batch;
    for (int j = 0; j < 4; ++j) {
        const int n = nb + j;
        if (n >= N) break;
        float* o = STz + (long long)n * lds + mb;
        if (VEC && mb + 3 < M) {
            *(f32x4*)o = f32x4{s[0][j], s[1][j], s[2][j], s[3][j]};
        } else {
            for (int i = 0; i < 4; ++i)
                if (mb + i < M) o[i] = s[i][j];
        }
    }
}

// One row per workgroup: G[row][c] := 2 g s^2 (rounded to T, in place) for c < cols, and sums[out_row] = sum_c of the stored values.
// Row `row` of matrix z (blockIdx.y) is sums entry row * batch + z: the default branch's S[k][b][b'] rows sum into entry b * K + k,
// the order of predicted_z's (b, k) rows.  blockIdx.z selects the (G, S, sums) or the (GT, ST, sumsT) set.
template <typename T>
__global__ __launch_bounds__(256) void diff_scores_bwd_kernel(T* __restrict__ G, const float* __restrict__ S, float* __restrict__ sums,
                                                              T* __restrict__ GT, const float* __restrict__ ST, float* __restrict__ sumsT,
                                                              int M, int N, int lds, long long s_batch, int batch) {
    const bool second = blockIdx.z == 1;
    const int rows = second ? N : M, cols = second ? M : N;
    const int row = blockIdx.x, z = blockIdx.y;
    if (row >= rows) return;
    T* g = (second ? GT : G) + z * s_batch + (long long)row * lds;
    const float* s = (second ? ST : S) + z * s_batch + (long long)row * lds;
    float part = 0.f;
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        const float sc = s[c];
        const T w = from_f32<T>(2.0f * to_f32(g[c]) * sc * sc);
        g[c] = w;
        part += to_f32(w);
    }
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (threadIdx.x == 0) (second ? sumsT : sums)[(long long)row * batch + z] = red[0] + red[1] + red[2] + red[3];
}

// out[row][e] -= mu[row] * X[row][e] for row < rows, e < E; rows of both at row_off(row, rpi, item, ld).
template <typename T>
__global__ __launch_bounds__(256) void diff_scores_rank1_kernel(const float* __restrict__ mu, const T* __restrict__ X, T* __restrict__ out,
                                                                int rows, int E, int rpi, long long item, long long ld) {
    const int row = blockIdx.x;
    if (row >= rows) return;
    const long long o = row_off(row, rpi, item, ld);
    const float m = mu[row];
    for (int e = threadIdx.x; e < E; e += blockDim.x)
        out[o + e] = from_f32<T>(fmaf(-m, to_f32(X[o + e]), to_f32(out[o + e])));
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
int launch_diff_scores_t(const void* P, const void* Tg, float* S, float* ST, int M, int N, int E, long long ldp, long long ldt, int t_rpi,
                         long long t_item, long long p_batch, long long t_batch, long long s_batch, int batch, int lds, hipStream_t stream) {
    constexpr int CH = Elem<T>::CH;
    // vector path: 16-byte operand loads need E, ldp, ldt, t_item, the batch strides and both base addresses in 16-byte units;
    // 16-byte score stores need lds, s_batch and S / ST aligned the same way
    const bool vec = E % CH == 0 && ldp % CH == 0 && ldt % CH == 0 && t_item % CH == 0 && p_batch % CH == 0 && t_batch % CH == 0 &&
                     aligned16(P) && aligned16(Tg) && lds % 4 == 0 && s_batch % 4 == 0 && aligned16(S) && (ST == nullptr || aligned16(ST));
    dim3 grid((N + DS_TILE - 1) / DS_TILE, (M + DS_TILE - 1) / DS_TILE, batch);
    if (vec)
        diff_scores_kernel<T, true><<<grid, 256, 0, stream>>>((const T*)P, (const T*)Tg, S, ST, M, N, E, ldp, ldt, t_rpi, t_item, p_batch,
                                                              t_batch, s_batch, lds);
    else
        diff_scores_kernel<T, false><<<grid, 256, 0, stream>>>((const T*)P, (const T*)Tg, S, ST, M, N, E, ldp, ldt, t_rpi, t_item, p_batch,
                                                               t_batch, s_batch, lds);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

}  // namespace

int launch_diff_scores(const void* P, const void* Tg, float* S, float* ST, int M, int N, int E, long long ldp, long long ldt, int t_rpi,
                       long long t_item, long long p_batch, long long t_batch, long long s_batch, int batch, int lds, int dtype,
                       hipStream_t stream) {
    if (dtype == CPC_DTYPE_BF16)
        return launch_diff_scores_t<bf16_t>(P, Tg, S, ST, M, N, E, ldp, ldt, t_rpi, t_item, p_batch, t_batch, s_batch, batch, lds, stream);
    return launch_diff_scores_t<float>(P, Tg, S, ST, M, N, E, ldp, ldt, t_rpi, t_item, p_batch, t_batch, s_batch, batch, lds, stream);
}

int launch_diff_scores_bwd(void* G, const float* S, float* sums, void* GT, const float* ST, float* sumsT, int M, int N, int lds,
                           long long s_batch, int batch, int dtype, hipStream_t stream) {
    const int two = GT != nullptr ? 2 : 1;
    dim3 grid(M > N ? M : N, batch, two);
    if (dtype == CPC_DTYPE_BF16)
        diff_scores_bwd_kernel<bf16_t><<<grid, 256, 0, stream>>>((bf16_t*)G, S, sums, (bf16_t*)GT, ST, sumsT, M, N, lds, s_batch, batch);
    else
        diff_scores_bwd_kernel<float><<<grid, 256, 0, stream>>>((float*)G, S, sums, (float*)GT, ST, sumsT, M, N, lds, s_batch, batch);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_diff_scores_rank1(const float* mu, const void* X, void* out, int rows, int E, int rpi, long long item, long long ld, int dtype,
                             hipStream_t stream) {
    const int threads = E >= 256 ? 256 : 64;
    if (dtype == CPC_DTYPE_BF16)
        diff_scores_rank1_kernel<bf16_t><<<rows, threads, 0, stream>>>(mu, (const bf16_t*)X, (bf16_t*)out, rows, E, rpi, item, ld);
    else
        diff_scores_rank1_kernel<float><<<rows, threads, 0, stream>>>(mu, (const float*)X, (float*)out, rows, E, rpi, item, ld);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
