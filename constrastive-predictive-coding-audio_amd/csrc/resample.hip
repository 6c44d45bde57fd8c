// Load-time conversion of audio files on the device (include/cpc_hip.h, cpc_resample; DESIGN.md, "Resampling and downmix at load"):
// channel downmix, rational resampling by L / M through a caller-made polyphase table, and the store as f32 or int16, for a list of
// segments (files) in one launch.  A workgroup makes one tile of RS_TILE consecutive outputs of one segment: it finds its segment by a
// uniform search in the tile prefix table, stages the downmixed, scaled input span of the tile once in LDS (zeros outside the segment's
// own frames, so no sample of a neighbouring file enters), and every lane then sums 2W + 1 products for each of its four outputs.
// Consecutive lanes make consecutive outputs (coalesced stores); their phases lie M apart, so the taps are kept transposed, [t][p]:
// at one t the 64 lanes of a wave read 64 floats of one L-float row, a few cache lines that stay in L1 / L2.  No atomics.
#include <cmath>
#include "cpc_common.h"
#include "cpc_kernels.h"
#include "../../include/cpc_hip.h"

namespace {

constexpr int RS_TILE = CPC_RESAMPLE_TILE;           // outputs per workgroup
constexpr int RS_THREADS = 256;
constexpr int RS_PER = RS_TILE / RS_THREADS;         // outputs per lane, RS_THREADS apart

// One downmixed frame: channel 0, or the mean of the C channels summed in channel order in f32.
template <typename S>
__device__ __forceinline__ float rs_frame(const S* __restrict__ f, int C, int mix) {
    float x = (float)f[0];
    if (mix) {
        for (int c = 1; c < C; ++c) x += (float)f[c];
        x /= (float)C;
    }
    return x;
}

__device__ __forceinline__ void rs_store(float* p, float v) { *p = v; }
// Half to even, saturated: the f32 value is the one the f32 store writes.
__device__ __forceinline__ void rs_store(short* p, float v) { *p = (short)(int)rintf(fminf(fmaxf(v, -32768.0f), 32767.0f)); }

template <typename S, typename D>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const S* __restrict__ src, long long src_frames_total, int C, int mix,
                                                              float in_scale, const float* __restrict__ taps, int L, int M, int W,
                                                              const long long* __restrict__ segs,
                                                              const long long* __restrict__ tile_first, int nseg, D* __restrict__ dst,
                                                              long long dst_total, float out_scale) {
    extern __shared__ float xs[];                    // the input span of the tile, downmixed and scaled
    // The last segment whose first tile is not behind this one (the same in every lane: scalar loads, a uniform loop).
    const long long b = blockIdx.x;
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_first[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const long long tile = b - tile_first[lo];
    const long long* e = segs + 4ll * lo;
    const long long s0 = e[0], N = e[1], d0 = e[2], Nout = e[3];
    // Guard: a segment that leaves [0, src_frames_total) or [0, dst_total), or a tile outside its segment, is skipped whole.
    if (tile < 0 || tile > (1ll << 40) / RS_TILE || s0 < 0 || N < 0 || N > src_frames_total - s0 || d0 < 0 || Nout < 0 ||
        Nout > dst_total - d0)
        return;
    const long long n0 = tile * RS_TILE;
    if (n0 >= Nout) return;
    const int cnt = (int)(Nout - n0 < RS_TILE ? Nout - n0 : RS_TILE);
    const long long a = n0 * M;                      // < 2^60: Nout <= dst_total <= 2^40, M <= 2^20
    const long long q0 = a / L;
    const int r0 = (int)(a - q0 * L);
    const int taps_n = 2 * W + 1;
    const int span = (int)(((long long)r0 + (long long)(cnt - 1) * M) / L) + taps_n;          // <= the LDS the launcher asked for
    const long long base = q0 - W;                   // the segment's frame behind xs[0]; may lie in front of the segment
    const S* seg_src = src + s0 * C;
    for (int j = threadIdx.x; j < span; j += RS_THREADS) {
        const long long i = base + j;
        float x = 0.0f;
        if (i >= 0 && i < N) x = rs_frame(seg_src + i * C, C, mix) * in_scale;
        xs[j] = x;
    }
    __syncthreads();
    int io[RS_PER], p[RS_PER];
    float acc[RS_PER];
#pragma unroll
    for (int k = 0; k < RS_PER; ++k) {
        int j = (int)threadIdx.x + k * RS_THREADS;
        j = j < cnt ? j : cnt - 1;                   // a lane behind the tile's end computes the last output again and stores nothing
        const unsigned u = (unsigned)r0 + (unsigned)j * (unsigned)M;          // < 2^31
        io[k] = (int)(u / (unsigned)L);
        p[k] = (int)(u - (unsigned)io[k] * (unsigned)L);
        acc[k] = 0.0f;
    }
    for (int t = 0; t < taps_n; ++t) {
        const float* row = taps + (long long)t * L;
#pragma unroll
        for (int k = 0; k < RS_PER; ++k) acc[k] = fmaf(row[p[k]], xs[io[k] + t], acc[k]);
    }
    D* out = dst + d0 + n0;
#pragma unroll
    for (int k = 0; k < RS_PER; ++k) {
        const int j = (int)threadIdx.x + k * RS_THREADS;
        if (j < cnt) rs_store(out + j, acc[k] * out_scale);
    }
}

}  // namespace

long long resample_span_floats(int L, int M, int W) { return ((long long)(RS_TILE - 1) * M) / L + 2ll * W + 2; }

int launch_resample(const void* src, int src_code, long long src_frames_total, int C, int mix, float in_scale, const float* taps, int L,
                    int M, int W, const long long* segs, const long long* tile_first, int nseg, long long ntiles, void* dst, int dst_code,
                    long long dst_total, float out_scale, hipStream_t stream) {
    const unsigned lds = (unsigned)(resample_span_floats(L, M, W) * sizeof(float));
    const dim3 grid((unsigned)ntiles);
#define RS_LAUNCH(S, D)                                                                                                               \
    resample_kernel<S, D><<<grid, RS_THREADS, lds, stream>>>((const S*)src, src_frames_total, C, mix, in_scale, taps, L, M, W, segs, \
                                                              tile_first, nseg, (D*)dst, dst_total, out_scale)
    if (src_code == 1 && dst_code == 1) RS_LAUNCH(short, short);
    else if (src_code == 1) RS_LAUNCH(short, float);
    else if (dst_code == 1) RS_LAUNCH(float, short);
    else RS_LAUNCH(float, float);
#undef RS_LAUNCH
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
