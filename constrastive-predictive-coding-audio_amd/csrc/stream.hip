// Whole-recording feature extraction (include/cpc_hip.h, cpc_stream_gather / cpc_feature_emit / cpc_stream_carry; DESIGN.md,
// "Whole-recording feature extraction"): R recordings ("streams") advance side by side, Tc frames per step, and one block of an
// int64 table [R][6] (first sample, samples, frames, first output row, recording, keep) says what every stream does in a step.
// Grid row r is stream r in all three kernels, so the reads of its table row are the same in every lane of a workgroup.
//   stream_gather   the samples of the step's windows as f32 rows, zeros behind a short window (dataset.hip's gather with a length)
//   feature_emit    the frames' z (the encoder's top rows) and c (the top recurrent layer's hidden states) into the feature stores,
//                   16 bytes of a source row per lane; with pooling, per (stream, block of 32 frames, channel) the f64 sum and sum
//                   of squares to a scratch, which feature_fold adds to the recordings' f64 accumulators in block order.  (f64 from
//                   the first addition: the square of an f32 value is exact in f64, and the deviation sqrt(E[x^2] - mean^2) loses
//                   half its digits to the rounding of the squares when they are formed in f32 -- seen as 2e-4 |mean| on a recording
//                   of one frame, whose deviation is 0.  The kernel is bound by its 16-byte loads, not by 2 CH f64 additions a row.)
//   stream_carry    the recurrent state a stream hands to its next step, or zeros where its recording ends
// All three are memory-bound: no LDS, no atomics; every sum has an order fixed by the arguments.
#include <cmath>
#include "cpc_common.h"
#include "cpc_draws.h"
#include "cpc_kernels.h"
#include "cpc_pieces.h"
#include "../../include/cpc_hip.h"

namespace {

constexpr int ROW = 6;          // int64 entries per table row
typedef __attribute__((ext_vector_type(2))) double f64x2;

// The guard of include/cpc_hip.h: a row that breaks one of the stated extents is idle.  (n <= L <= 2^24 and nf <= Tc, so the
// differences cannot overflow.)
__device__ __forceinline__ bool stream_row_ok(const long long* __restrict__ row, const StreamExtents& x) {
    const long long first = row[0], n = row[1], nf = row[2], out = row[3], rec = row[4];
    return rec >= 0 && rec < x.n_rec && n >= 0 && n <= x.L && first >= 0 && first <= x.store_len - n && nf >= 0 && nf <= x.Tc &&
           out >= 0 && out <= x.total_frames - nf;
}

// ------------------------------------------------------------------------------------------------------------------ gather
// Workgroup (blockIdx.x, blockIdx.y): outputs [tile blockIdx.x, +tile) of row blockIdx.y, tile = 4 ITERS blockDim.x; a lane ITERS pieces
// of 4, blockDim.x pieces apart.  Outputs [0, n) are samples first .. first + n - 1, outputs [n, L) zeros; an idle row has n = 0.
template <typename T, bool COPY, int ITERS>
__global__ __launch_bounds__(256) void stream_gather_kernel(const T* __restrict__ store, const long long* __restrict__ table,
                                                            StreamExtents ext, float* __restrict__ out, long long ldo, float scale,
                                                            int vec_out) {
    const int r = blockIdx.y, L = ext.L;
    const long long* row = table + (long long)r * ROW;
    const bool ok = stream_row_ok(row, ext);
    const int n = ok ? (int)row[1] : 0;
    const T* src = store + (ok ? row[0] : 0);
    float* dst = out + (long long)r * ldo;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int n0 = WG_PIECE * (((int)blockIdx.x * ITERS + it) * (int)blockDim.x + (int)threadIdx.x);
        if (n0 >= L) continue;
        float v[WG_PIECE] = {0.f, 0.f, 0.f, 0.f};
        if (n0 + WG_PIECE - 1 < n) {
            const WgPiece<T> p = wg_load(src + n0);
#pragma unroll
            for (int j = 0; j < WG_PIECE; ++j) v[j] = wg_value<T, COPY>(p.v[j], scale);
        } else {
#pragma unroll
            for (int j = 0; j < WG_PIECE; ++j)
                if (n0 + j < n) v[j] = wg_value<T, COPY>(src[n0 + j], scale);
        }
        if (vec_out && n0 + WG_PIECE - 1 < L) {
            *(f32x4*)(dst + n0) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int j = 0; j < WG_PIECE; ++j)
                if (n0 + j < L) dst[n0 + j] = v[j];
        }
    }
}

template <typename T, bool COPY>
void stream_gather_launch(const void* store, const long long* table, const StreamExtents& ext, float* out, int R, long long ldo,
                          float scale, hipStream_t stream) {
    const int vec_out = aligned16(out) && ldo % 4 == 0;
    const T* st = (const T*)store;
    const int L = ext.L;
    // (cpc_window_gather's grid rule: tiles of 4096, 1024 or 256 outputs, the largest that still gives 1024 workgroups)
    const long long want = 1024;
    auto tiles = [&](int tile) { return (long long)R * ((L + tile - 1) / tile); };
    if (tiles(4096) >= want)
        stream_gather_kernel<T, COPY, 4><<<dim3((L + 4095) / 4096, R), 256, 0, stream>>>(st, table, ext, out, ldo, scale, vec_out);
    else if (tiles(1024) >= want)
        stream_gather_kernel<T, COPY, 1><<<dim3((L + 1023) / 1024, R), 256, 0, stream>>>(st, table, ext, out, ldo, scale, vec_out);
    else
        stream_gather_kernel<T, COPY, 1><<<dim3((L + 255) / 256, R), 64, 0, stream>>>(st, table, ext, out, ldo, scale, vec_out);
}

// -------------------------------------------------------------------------------------------------------------------- emit
// One 16-byte piece of a source row: stored as U (the same bits for U = T, round-to-nearest-even to bf16, exact to f32) and widened
// to f32 for the pooled sums.
template <typename T, typename U>
__device__ __forceinline__ void emit_piece(const T* __restrict__ src, U* __restrict__ dst, float (&v)[Elem<T>::CH]) {
    if constexpr (sizeof(T) == 4) {
        const uint4 raw = *(const uint4*)src;
        const f32x4 f = __builtin_bit_cast(f32x4, raw);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = f[e];
        if constexpr (sizeof(U) == 4) *(uint4*)dst = raw;
        else store4(dst, f);
    } else {
        const uint4 raw = *(const uint4*)src;
        const bf16x8 h = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)h[e];
        if constexpr (sizeof(U) == 2) {
            *(uint4*)dst = raw;
        } else {
            *(f32x4*)dst = f32x4{v[0], v[1], v[2], v[3]};
            *(f32x4*)(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
        }
    }
}

// Workgroup (blockIdx.x, blockIdx.y, blockIdx.z): frames [32 blockIdx.y, +32) of stream blockIdx.z; a lane owns one 16-byte piece of
// the channels -- the pieces of z first, then those of c -- and walks the block's frames in order, so that neighbouring lanes read
// neighbouring 16 bytes of every row.  partial: [R][nblk][2][E + H] f64, sums in row 0 and sums of squares in row 1 of a block.
template <typename T, typename U>
__global__ __launch_bounds__(256) void feature_emit_kernel(const long long* __restrict__ table, StreamExtents ext,
                                                           const T* __restrict__ top, long long top_item, const T* __restrict__ hall,
                                                           long long hall_item, U* __restrict__ z_out, U* __restrict__ c_out, int E, int H,
                                                           double* __restrict__ partial, int nblk) {
    constexpr int CH = Elem<T>::CH;
    const int r = blockIdx.z;
    const long long* row = table + (long long)r * ROW;
    if (!stream_row_ok(row, ext)) return;
    const int nf = (int)row[2], f0 = (int)blockIdx.y * CPC_EMIT_FRAMES;
    if (f0 >= nf) return;
    const int pz = z_out ? E / CH : 0, pc = c_out ? H / CH : 0;
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= pz + pc) return;
    const bool is_z = q < pz;
    const int C = is_z ? E : H, ch = (is_z ? q : q - pz) * CH;
    // frame t of the stream: row t of its top rows, row t + 1 of its hidden states (row 0 is the state the step started from)
    const T* src = (is_z ? top + (long long)r * top_item : hall + (long long)r * hall_item + H) + (long long)f0 * C + ch;
    U* dst = (is_z ? z_out : c_out) + (row[3] + f0) * C + ch;
    const int count = min(CPC_EMIT_FRAMES, nf - f0);
    double s[CH], ss[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) s[e] = ss[e] = 0.0;
    for (int t = 0; t < count; ++t) {
        float v[CH];
        emit_piece<T, U>(src + (long long)t * C, dst + (long long)t * C, v);
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            const double d = (double)v[e];
            s[e] += d;
            ss[e] += d * d;
        }
    }
    if (partial) {
        double* p = partial + (((long long)r * nblk + blockIdx.y) * 2) * (E + H) + (is_z ? 0 : E) + ch;
#pragma unroll
        for (int e = 0; e < CH; e += 2) {
            *(f64x2*)(p + e) = f64x2{s[e], s[e + 1]};
            *(f64x2*)(p + (E + H) + e) = f64x2{ss[e], ss[e + 1]};
        }
    }
}

// The partial sums of a step into the accumulators acc [n_rec][2][C] f64 of the streams' recordings: a lane owns one channel of one
// stream and adds its blocks in block order.  A recording is owned by one stream in a step, and steps are ordered by the stream.
__global__ __launch_bounds__(256) void feature_fold_kernel(const long long* __restrict__ table, StreamExtents ext,
                                                           const double* __restrict__ partial, int nblk, int E, int H,
                                                           double* __restrict__ acc_z, double* __restrict__ acc_c) {
    const int r = blockIdx.y;
    const long long* row = table + (long long)r * ROW;
    if (!stream_row_ok(row, ext)) return;
    const int nb = ((int)row[2] + CPC_EMIT_FRAMES - 1) / CPC_EMIT_FRAMES;
    const int col = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (nb == 0 || col >= E + H) return;
    const bool is_z = col < E;
    double* acc = is_z ? acc_z : acc_c;
    if (!acc) return;
    const int C = is_z ? E : H, ch = is_z ? col : col - E;
    double* a = acc + (row[4] * 2) * C + ch;
    double s = a[0], q = a[C];
    const double* p = partial + ((long long)r * nblk * 2) * (E + H) + col;
    for (int b = 0; b < nb; ++b) {
        s += p[(long long)(2 * b) * (E + H)];
        q += p[(long long)(2 * b + 1) * (E + H)];
    }
    a[0] = s;
    a[C] = q;
}

template <typename T, typename U>
void feature_emit_launch(const long long* table, const StreamExtents& ext, const void* top, long long top_item, const void* hall,
                         long long hall_item, void* z_out, void* c_out, int R, int E, int H, double* partial, hipStream_t stream) {
    constexpr int CH = Elem<T>::CH;
    const int pieces = (z_out ? E / CH : 0) + (c_out ? H / CH : 0);
    const int threads = min(256, (pieces + 63) / 64 * 64);
    const int nblk = (ext.Tc + CPC_EMIT_FRAMES - 1) / CPC_EMIT_FRAMES;
    feature_emit_kernel<T, U><<<dim3((pieces + threads - 1) / threads, nblk, R), threads, 0, stream>>>(
        table, ext, (const T*)top, top_item, (const T*)hall, hall_item, (U*)z_out, (U*)c_out, E, H, partial, nblk);
}

// ------------------------------------------------------------------------------------------------------------------- carry
struct CarryPointers {
    const float* src[CPC_STREAM_MAX_STATES];
    float* dst[CPC_STREAM_MAX_STATES];
};

// Workgroup (blockIdx.x, blockIdx.y, blockIdx.z): 64 pieces of four floats of stream blockIdx.y's row of state array blockIdx.z.
__global__ __launch_bounds__(64) void stream_carry_kernel(const long long* __restrict__ table, StreamExtents ext, CarryPointers p, int H) {
    const int r = blockIdx.y, j = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= H) return;
    const long long* row = table + (long long)r * ROW;
    const bool keep = stream_row_ok(row, ext) && row[5] == 1;
    const long long at = (long long)r * H + j;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (keep) v = *(const f32x4*)(p.src[blockIdx.z] + at);
    *(f32x4*)(p.dst[blockIdx.z] + at) = v;
}

}  // namespace

int launch_stream_gather(const void* store, int store_code, const long long* table, const StreamExtents& ext, float* out, int R,
                         long long ldo, float scale, hipStream_t stream) {
    if (store_code == 1)
        stream_gather_launch<short, false>(store, table, ext, out, R, ldo, scale, stream);
    else if (scale == 1.0f)
        stream_gather_launch<float, true>(store, table, ext, out, R, ldo, scale, stream);
    else
        stream_gather_launch<float, false>(store, table, ext, out, R, ldo, scale, stream);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_feature_emit(const long long* table, const StreamExtents& ext, const void* top, long long top_item, const void* hall,
                        long long hall_item, int src_dtype, void* z_out, void* c_out, int out_dtype, int R, int E, int H, double* partial,
                        double* acc_z, double* acc_c, hipStream_t stream) {
    const bool sb = src_dtype == CPC_DTYPE_BF16, ob = out_dtype == CPC_DTYPE_BF16;
#define EMIT(T, U) feature_emit_launch<T, U>(table, ext, top, top_item, hall, hall_item, z_out, c_out, R, E, H, partial, stream)
    if (sb && ob) EMIT(bf16_t, bf16_t);
    else if (sb) EMIT(bf16_t, float);
    else if (ob) EMIT(float, bf16_t);
    else EMIT(float, float);
#undef EMIT
    CPC_CHECK_LAUNCH();
    if (partial) {
        const int nblk = (ext.Tc + CPC_EMIT_FRAMES - 1) / CPC_EMIT_FRAMES;
        feature_fold_kernel<<<dim3((E + H + 255) / 256, R), 256, 0, stream>>>(table, ext, partial, nblk, E, H, z_out ? acc_z : nullptr,
                                                                            c_out ? acc_c : nullptr);
        CPC_CHECK_LAUNCH();
    }
    return CPC_OK;
}

int launch_stream_carry(const long long* table, const StreamExtents& ext, const float* const* src, float* const* dst, int nstate, int R,
                        int H, hipStream_t stream) {
    CarryPointers p = {};
    for (int i = 0; i < nstate; ++i) {
        p.src[i] = src[i];
        p.dst[i] = dst[i];
    }
    stream_carry_kernel<<<dim3((H / 4 + 63) / 64, R, nstate), 64, 0, stream>>>(table, ext, p, H);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
