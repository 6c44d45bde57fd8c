// Row normalisation for the cosine-similarity ("normalized") scores and its backward (include/cpc_hip.h, cpc_norm_rows /
// cpc_norm_rows_bwd; cpc_norm_rows_dev / cpc_norm_rows_bwd_dev with the scale in device memory, and the temperature's own update,
// cpc_temperature_step / cpc_temperature_set).  Memory-bound: one wave per row, the row held in registers between the reduction and
// the scaling, so every row is read once and written once.  The sums have one fixed order (a lane's own elements in storage order,
// then an xor-shuffle butterfly): no atomics, no LDS, no dependence on the grid, and every lane of the wave ends with the same bits.
// (The temperature's update adds the per-row dots in one workgroup, through a fixed LDS tree.)
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

// Where a kernel takes its scale from, and whether the backward also leaves the per-row dot products: HostScale is the launch argument of
// cpc_norm_rows / cpc_norm_rows_bwd (one float in the kernel's argument block, as before the _dev entry points existed), DevScale reads
// scale[0] from device memory (cpc_norm_rows_dev / cpc_norm_rows_bwd_dev: a temperature a captured step can change) and carries ``dots``.
struct HostScale {
    float v;
    static constexpr bool DOTS = false;
    __device__ __forceinline__ float get() const { return v; }
    __device__ __forceinline__ void put_dot(int, float) const {}
};
struct DevScale {
    const float* p;
    float* dots;
    static constexpr bool DOTS = true;
    __device__ __forceinline__ float get() const { return p[0]; }
    __device__ __forceinline__ void put_dot(int row, float d) const { dots[row] = d; }
};

// inv[row] = 1 / max(|X[row]|, eps) and Y[row] = X[row] * (scale * inv[row]); rows at row_off(row, rpi, item, ld) of X and Y.
// (n < eps ? eps : n, not fmaxf: a NaN norm stays NaN, as torch's clamp_min keeps it.)
template <typename T, int NP, bool VEC, typename S>
__global__ __launch_bounds__(64 * NR_WAVES) void norm_rows_kernel(const T* X, T* Y, float* __restrict__ inv, int rows, int E, int rpi,
                                                                   long long item, long long ld, S scale_src, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * NR_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;            // (whole waves leave: the shuffles below see 64 live lanes)
    const long long o = row_off(row, rpi, item, ld);
    Row<T, NP, VEC> x;
    x.load(X + o, E, lane);
    const float n = sqrtf(wave_dot(x, x));
    const float r = 1.0f / (n < eps ? eps : n);
    const float c = scale_src.get() * r;
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int j = 0; j < Row<T, NP, VEC>::CH; ++j) x.v[p][j] *= c;
    x.tail *= c;
    x.store(Y + o, E, lane);
    if (lane == 0) inv[row] = r;
}

// G[row] := scale inv[row] G[row] - (inv[row] / scale) <Y[row], G[row]> Y[row]; the second term only where inv[row] < 1 / eps.
// DevScale: dots[row] = <Y[row], G[row]> of the stored values, in both branches (a clamped row still carries the scale), taken before G
// is overwritten: d loss / d log(scale) is the sum of them (cpc_temperature_step).
template <typename T, int NP, bool VEC, typename S>
__global__ __launch_bounds__(64 * NR_WAVES) void norm_rows_bwd_kernel(const T* __restrict__ Y, const float* __restrict__ inv,
                                                                       T* __restrict__ G, int rows, int E, int rpi, long long item,
                                                                       long long ld, S scale_src, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * NR_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long o = row_off(row, rpi, item, ld);
    const float scale = scale_src.get();
    Row<T, NP, VEC> y, g;
    y.load(Y + o, E, lane);
    g.load(G + o, E, lane);
    const float r = inv[row];
    const float c1 = scale * r;
    if (r >= 1.0f / eps) {              // the norm was clamped: y = x * scale / eps, no projection term
        if (S::DOTS) {
            const float d = wave_dot(y, g);
            if (lane == 0) scale_src.put_dot(row, d);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int j = 0; j < Row<T, NP, VEC>::CH; ++j) g.v[p][j] *= c1;
        g.tail *= c1;
    } else {
        const float d = wave_dot(y, g);
        if (S::DOTS && lane == 0) scale_src.put_dot(row, d);
        const float c2 = (r / scale) * d;
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int j = 0; j < Row<T, NP, VEC>::CH; ++j) g.v[p][j] = fmaf(-c2, y.v[p][j], c1 * g.v[p][j]);
        g.tail = fmaf(-c2, y.tail, c1 * g.tail);
    }
    g.store(G + o, E, lane);
}

// ---- the temperature as device state (include/cpc_hip.h: cpc_temperature_step, cpc_temperature_set) ----
// tstate f32[8] = {s = log(scale), scale = exp(s), Adam's m, v of s, the latest d loss / d s, tau = 1 / scale, 0, 0}.
constexpr int TS_THREADS = 256;

// d loss / d s = grad_scale * sum of dots[0 .. rows), then torch.optim.Adam's update of the one scalar s (adam_update's expressions of
// pointwise.hip, without decay), the clamp to [s_min, s_max] and the two derived values.  One workgroup: thread i adds dots[i],
// dots[i + 256], ... in that order, an LDS tree with a fixed shape follows: the same data give the same bits.  With ``state`` (the f32[4] of
// cpc_adam_dev / cpc_adamw_dev, already advanced by this step's update) the step size is state[1] * step_size and the second-moment
// correction state[2]; otherwise both are the arguments.
__global__ __launch_bounds__(TS_THREADS) void temperature_step_kernel(float* __restrict__ tstate, const float* __restrict__ dots, int rows,
                                                                      float step_size, float inv_bc2_sqrt, float b1, float b2, float eps,
                                                                      const float* __restrict__ state, float grad_scale, float s_min,
                                                                      float s_max, const float* __restrict__ skip) {
    if (skip && skip[0] != 0.f) return;          // the NaN guard of the update this launch follows: nothing is written
    __shared__ float part[TS_THREADS];
    float acc = 0.f;
    for (int i = threadIdx.x; i < rows; i += TS_THREADS) acc += dots[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int off = TS_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (state) { step_size = state[1] * step_size; inv_bc2_sqrt = state[2]; }
    const float g = grad_scale * part[0];
    float s = tstate[0], m = tstate[2], v = tstate[3];
    m = m + (g - m) * (1.f - b1);
    v = v * b2 + (1.f - b2) * g * g;
    s = s - step_size * (m / (sqrtf(v) * inv_bc2_sqrt + eps));
    s = s < s_min ? s_min : (s > s_max ? s_max : s);          // (a NaN stays NaN: the run's NaN guard is the loss's)
    tstate[0] = s;
    tstate[1] = (float)exp((double)s);
    tstate[2] = m;
    tstate[3] = v;
    tstate[4] = g;
    tstate[5] = (float)exp(-(double)s);
}

// The scheduled temperature of the 0-based step ``step`` (with ``state``: step_offset + the device's step count, the steps finished so
// far), in double as lr_factor of pointwise.hip: q = min(step / total, 1); kind 0 linear, 1 cosine.
__global__ void temperature_set_kernel(float* __restrict__ tstate, int kind, double start, double end, long long total, long long step,
                                       const float* __restrict__ state, long long step_offset) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (state) step = step_offset + (long long)__float_as_int(state[0]);
    const double q = fmin((double)step / (double)total, 1.0);
    const double tau = kind == 0 ? start + (end - start) * q : end + (start - end) * (0.5 * (1.0 + cos(3.14159265358979323846 * q)));
    const float scale = (float)(1.0 / tau);
    tstate[0] = (float)log((double)scale);
    tstate[1] = scale;
    tstate[5] = (float)tau;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T, int NP, bool VEC, typename S>
void launch_np(bool bwd, const void* A, float* inv, void* Bp, int rows, int E, int rpi, long long item, long long ld, S scale,
               float eps, hipStream_t stream) {
    const dim3 grid((rows + NR_WAVES - 1) / NR_WAVES), block(64 * NR_WAVES);
    if (bwd)
        norm_rows_bwd_kernel<T, NP, VEC, S><<<grid, block, 0, stream>>>((const T*)A, inv, (T*)Bp, rows, E, rpi, item, ld, scale, eps);
    else
        norm_rows_kernel<T, NP, VEC, S><<<grid, block, 0, stream>>>((const T*)A, (T*)Bp, inv, rows, E, rpi, item, ld, scale, eps);
}

// A: X (forward) / Y (backward); Bp: Y (forward) / G (backward).  NP: the smallest power of two with 64 NP CH >= E.
template <typename T, typename S>
int launch_t(bool bwd, const void* A, float* inv, void* Bp, int rows, int E, int rpi, long long item, long long ld, S scale, float eps,
             hipStream_t stream) {
    constexpr int CH = Elem<T>::CH;
    const bool vec = aligned16(A) && aligned16(Bp) && ld % CH == 0 && (rpi == 0 || item % CH == 0);
    const int need = (E + 64 * CH - 1) / (64 * CH);
#define NR_CASE(NP)                                                                                     \
    if (need <= NP) {                                                                                   \
        if (vec) launch_np<T, NP, true, S>(bwd, A, inv, Bp, rows, E, rpi, item, ld, scale, eps, stream);   \
        else launch_np<T, NP, false, S>(bwd, A, inv, Bp, rows, E, rpi, item, ld, scale, eps, stream);      \
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
    if (dtype == CPC_DTYPE_BF16) return launch_t<bf16_t>(false, X, inv, Y, rows, E, rpi, item, ld, HostScale{scale}, eps, stream);
    return launch_t<float>(false, X, inv, Y, rows, E, rpi, item, ld, HostScale{scale}, eps, stream);
}

int launch_norm_rows_bwd(const void* Y, const float* inv, void* G, int rows, int E, int rpi, long long item, long long ld, float scale,
                         float eps, int dtype, hipStream_t stream) {
    if (dtype == CPC_DTYPE_BF16)
        return launch_t<bf16_t>(true, Y, const_cast<float*>(inv), G, rows, E, rpi, item, ld, HostScale{scale}, eps, stream);
    return launch_t<float>(true, Y, const_cast<float*>(inv), G, rows, E, rpi, item, ld, HostScale{scale}, eps, stream);
}

int launch_norm_rows_dev(const void* X, void* Y, float* inv, int rows, int E, int rpi, long long item, long long ld, const float* scale,
                         float eps, int dtype, hipStream_t stream) {
    const DevScale s{scale, nullptr};
    if (dtype == CPC_DTYPE_BF16) return launch_t<bf16_t>(false, X, inv, Y, rows, E, rpi, item, ld, s, eps, stream);
    return launch_t<float>(false, X, inv, Y, rows, E, rpi, item, ld, s, eps, stream);
}

int launch_norm_rows_bwd_dev(const void* Y, const float* inv, void* G, float* dots, int rows, int E, int rpi, long long item, long long ld,
                             const float* scale, float eps, int dtype, hipStream_t stream) {
    const DevScale s{scale, dots};
    if (dtype == CPC_DTYPE_BF16) return launch_t<bf16_t>(true, Y, const_cast<float*>(inv), G, rows, E, rpi, item, ld, s, eps, stream);
    return launch_t<float>(true, Y, const_cast<float*>(inv), G, rows, E, rpi, item, ld, s, eps, stream);
}

int launch_temperature_step(float* tstate, const float* dots, int rows, float lr, float b1, float b2, float eps, int step,
                            const float* adam_state, float grad_scale, float s_min, float s_max, const float* skip, hipStream_t stream) {
    float step_size = lr, inv_bc2_sqrt = 1.f;
    if (!adam_state) {          // the bias corrections in double, rounded once (launch_adam's expressions)
        const double bc1 = 1.0 - pow((double)b1, step), bc2 = 1.0 - pow((double)b2, step);
        step_size = (float)((double)lr / bc1);
        inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    }
    temperature_step_kernel<<<dim3(1), dim3(TS_THREADS), 0, stream>>>(tstate, dots, rows, step_size, inv_bc2_sqrt, b1, b2, eps, adam_state,
                                                                      grad_scale, s_min, s_max, skip);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_temperature_set(float* tstate, int kind, double start, double end, long long total_steps, long long step,
                           const float* adam_state, long long step_offset, hipStream_t stream) {
    temperature_set_kernel<<<dim3(1), dim3(64), 0, stream>>>(tstate, kind, start, end, total_steps, step, adam_state, step_offset);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
