// Row normalisation for the cosine-similarity ("normalized") scores and its backward (include/cpc_hip.h, cpc_norm_rows /
// cpc_norm_rows_bwd).  Memory-bound: one wave per row, the row held in registers between the reduction and the scaling, so every
// row is read once and written once.  The sums have one fixed order (a lane's own elements in storage order, then an xor-shuffle
// butterfly): no atomics, no LDS, no dependence on the grid, and every lane of the wave ends with the same bits.
#include <cmath>
#include "cpc_common.h"
#include "cpc_kernels.h"

namespace {

constexpr int NR_WAVES = 4;        // rows per workgroup, one wave each

// 16-byte pieces: CH elements of a row as f32
__device__ __forceinline__ void load_piece(const float* src, float (&v)[4]) {
    const f32x4 x = *(const f32x4*)src;
    v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
}
__device__ __forceinline__ void load_piece(const bf16_t* src, float (&v)[8]) {
    const bf16x8 x = *(const bf16x8*)src;
    for (int j = 0; j < 8; ++j) v[j] = (float)x[j];
}
__device__ __forceinline__ void store_piece(float* dst, const float (&v)[4]) { *(f32x4*)dst = f32x4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void store_piece(bf16_t* dst, const float (&v)[8]) {
    bf16x8 o;
    for (int j = 0; j < 8; ++j) o[j] = (bf16_t)v[j];
    *(bf16x8*)dst = o;
}

// What a lane holds of one row: NP pieces of CH elements (+ one tail element), zeros where the row has ended.
//   VEC   piece p = elements [(64 p + lane) CH, +CH): one 16-byte load, contiguous over the wave; the E % CH elements behind the last
//         whole piece go one to a lane (tail).  Needs 16-byte aligned row starts.
//   !VEC  element j of piece p = element (p CH + j) 64 + lane (scalar loads, contiguous over the wave); no tail.
template <typename T, int NP, bool VEC>
struct Row {
    static constexpr int CH = Elem<T>::CH;
    float v[NP][CH];
    float tail;

    __device__ __forceinline__ void load(const T* row, int E, int lane) {
        tail = 0.f;
        if (VEC) {
            const int EV = E - E % CH;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int e = (p * 64 + lane) * CH;
                if (e < EV) {
                    load_piece(row + e, v[p]);
                } else {
#pragma unroll
                    for (int j = 0; j < CH; ++j) v[p][j] = 0.f;
                }
            }
            if (lane < E - EV) tail = to_f32(row[EV + lane]);
        } else {
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const int e = (p * CH + j) * 64 + lane;
                    v[p][j] = e < E ? to_f32(row[e]) : 0.f;
                }
        }
    }

    __device__ __forceinline__ void store(T* row, int E, int lane) const {
        if (VEC) {
            const int EV = E - E % CH;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int e = (p * 64 + lane) * CH;
                if (e < EV) store_piece(row + e, v[p]);
            }
            if (lane < E - EV) row[EV + lane] = from_f32<T>(tail);
        } else {
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const int e = (p * CH + j) * 64 + lane;
                    if (e < E) row[e] = from_f32<T>(v[p][j]);
                }
        }
    }
};

// sum over the wave of a lane's a . b: an fma chain over the lane's elements in storage order, the tail last, then the butterfly
template <typename T, int NP, bool VEC>
__device__ __forceinline__ float wave_dot(const Row<T, NP, VEC>& a, const Row<T, NP, VEC>& b) {
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int j = 0; j < Row<T, NP, VEC>::CH; ++j) s = fmaf(a.v[p][j], b.v[p][j], s);
    s = fmaf(a.tail, b.tail, s);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// inv[row] = 1 / max(|X[row]|, eps) and Y[row] = X[row] * (scale * inv[row]); rows at row_off(row, rpi, item, ld) of X and Y.
// (n < eps ? eps : n, not fmaxf: a NaN norm stays NaN, as torch's clamp_min keeps it.)
template <typename T, int NP, bool VEC>
__global__ __launch_bounds__(64 * NR_WAVES) void norm_rows_kernel(const T* X, T* Y, float* __restrict__ inv, int rows, int E, int rpi,
                                                                   long long item, long long ld, float scale, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * NR_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;            // (whole waves leave: the shuffles below see 64 live lanes)
    const long long o = row_off(row, rpi, item, ld);
    Row<T, NP, VEC> x;
    x.load(X + o, E, lane);
    const float n = sqrtf(wave_dot(x, x));
    const float r = 1.0f / (n < eps ? eps : n);
    const float c = scale * r;
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int j = 0; j < Row<T, NP, VEC>::CH; ++j) x.v[p][j] *= c;
    x.tail *= c;
    x.store(Y + o, E, lane);
    if (lane == 0) inv[row] = r;
}

// G[row] := scale inv[row] G[row] - (inv[row] / scale) <Y[row], G[row]> Y[row]; the second term only where inv[row] < 1 / eps.
template <typename T, int NP, bool VEC>
__global__ __launch_bounds__(64 * NR_WAVES) void norm_rows_bwd_kernel(const T* __restrict__ Y, const float* __restrict__ inv,
                                                                       T* __restrict__ G, int rows, int E, int rpi, long long item,
                                                                       long long ld, float scale, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * NR_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long o = row_off(row, rpi, item, ld);
    Row<T, NP, VEC> y, g;
    y.load(Y + o, E, lane);
    g.load(G + o, E, lane);
    const float r = inv[row];
    const float c1 = scale * r;
    if (r >= 1.0f / eps) {              // the norm was clamped: y = x * scale / eps, no projection term
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int j = 0; j < Row<T, NP, VEC>::CH; ++j) g.v[p][j] *= c1;
        g.tail *= c1;
    } else {
        const float c2 = (r / scale) * wave_dot(y, g);
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int j = 0; j < Row<T, NP, VEC>::CH; ++j) g.v[p][j] = fmaf(-c2, y.v[p][j], c1 * g.v[p][j]);
        g.tail = fmaf(-c2, y.tail, c1 * g.tail);
    }
    g.store(G + o, E, lane);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T, int NP, bool VEC>
void launch_np(bool bwd, const void* A, float* inv, void* Bp, int rows, int E, int rpi, long long item, long long ld, float scale,
               float eps, hipStream_t stream) {
    const dim3 grid((rows + NR_WAVES - 1) / NR_WAVES), block(64 * NR_WAVES);
    if (bwd)
        norm_rows_bwd_kernel<T, NP, VEC><<<grid, block, 0, stream>>>((const T*)A, inv, (T*)Bp, rows, E, rpi, item, ld, scale, eps);
    else
        norm_rows_kernel<T, NP, VEC><<<grid, block, 0, stream>>>((const T*)A, (T*)Bp, inv, rows, E, rpi, item, ld, scale, eps);
}

// A: X (forward) / Y (backward); Bp: Y (forward) / G (backward).  NP: the smallest power of two with 64 NP CH >= E.
template <typename T>
int launch_t(bool bwd, const void* A, float* inv, void* Bp, int rows, int E, int rpi, long long item, long long ld, float scale, float eps,
             hipStream_t stream) {
    constexpr int CH = Elem<T>::CH;
    const bool vec = aligned16(A) && aligned16(Bp) && ld % CH == 0 && (rpi == 0 || item % CH == 0);
    const int need = (E + 64 * CH - 1) / (64 * CH);
#define NR_CASE(NP)                                                                                     \
    if (need <= NP) {                                                                                   \
        if (vec) launch_np<T, NP, true>(bwd, A, inv, Bp, rows, E, rpi, item, ld, scale, eps, stream);   \
        else launch_np<T, NP, false>(bwd, A, inv, Bp, rows, E, rpi, item, ld, scale, eps, stream);      \
        CPC_CHECK_LAUNCH();                                                                             \
        return CPC_OK;                                                                                  \
    }
    NR_CASE(1)
    NR_CASE(2)
    NR_CASE(4)
    NR_CASE(8)
    if constexpr (CH == 4) {            // f32 only: E in (2048, 4096]
        NR_CASE(16)
    }
#undef NR_CASE
    return CPC_EINVAL;
}

}  // namespace

int launch_norm_rows(const void* X, void* Y, float* inv, int rows, int E, int rpi, long long item, long long ld, float scale, float eps,
                     int dtype, hipStream_t stream) {
    if (dtype == CPC_DTYPE_BF16) return launch_t<bf16_t>(false, X, inv, Y, rows, E, rpi, item, ld, scale, eps, stream);
    return launch_t<float>(false, X, inv, Y, rows, E, rpi, item, ld, scale, eps, stream);
}

int launch_norm_rows_bwd(const void* Y, const float* inv, void* G, int rows, int E, int rpi, long long item, long long ld, float scale,
                         float eps, int dtype, hipStream_t stream) {
    if (dtype == CPC_DTYPE_BF16) return launch_t<bf16_t>(true, Y, const_cast<float*>(inv), G, rows, E, rpi, item, ld, scale, eps, stream);
    return launch_t<float>(true, Y, const_cast<float*>(inv), G, rows, E, rpi, item, ld, scale, eps, stream);
}
