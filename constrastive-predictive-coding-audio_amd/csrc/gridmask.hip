// Masking augmentation on the channels-last input grid of the scalogram engine (include/cpc_hip.h, cpc_grid_sum / cpc_grid_mask;
// DESIGN.md, "Grid masking"): up to 8 frequency bands and 8 time spans of every clip's [W][H][Cc] grid are filled with zero, a
// constant or the clip's own per-channel mean.  The draws are those of the waveform augmentation (cpc_draws.h) at fields of their own,
// so a launch has no state and the host restates every span.  The in-place form (the trainer's) is launched over the mask
// rectangles and reads no grid element; the copy form sweeps the grid once.  No atomics, every sum in one fixed order.
#include <cmath>
#include "cpc_common.h"
#include "cpc_draws.h"
#include "cpc_kernels.h"
#include "../../include/cpc_hip.h"

namespace {

constexpr int GM_THREADS = 256;
constexpr int GS_CHUNK = 4096;                        // elements per partial sum: 256 threads x 4 pieces x 4 floats
constexpr u64 GM_FIELD = 0x4D41534Bull;               // the mask fields start here, clear of every field of the waveform augmentation
constexpr int GM_COPY_ITERS = 8;                      // pieces of 4 elements a lane of the copy form moves (the per-clip draws are per workgroup)
constexpr int GM_RECT_ITERS = 4;                      // pieces of 4 elements a lane of the in-place form may store

// partial[b][c][ch] = sum of channel ch over x[b][4096 c .. min(4096 (c + 1), n)).  Element e of a clip holds channel e % CC, and a
// lane's pieces start at multiples of 4, so position j of every piece holds channel j % CC.  Thread t: a[j] = the chain over p = 0 .. 3
// of element 4 (256 p + t) + j (zeros behind n leave a chain's value as it is), then the positions of one channel are combined, then
// the butterfly, then the four waves.  VEC only changes how the same elements are loaded.
template <int CC, bool VEC>
__global__ __launch_bounds__(GM_THREADS) void grid_sum_kernel(const float* __restrict__ x, float* __restrict__ partial, long long ldb,
                                                              unsigned n, int chunks) {
    __shared__ float wave_sum[GM_THREADS / 64][CC];
    const int c = blockIdx.x, b = blockIdx.y;
    const float* row = x + (long long)b * ldb;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const unsigned e = (unsigned)c * GS_CHUNK + 4u * (unsigned)(p * GM_THREADS + (int)threadIdx.x);
        float v[4];
        if (VEC && e + 3u < n) {
            const f32x4 q = *(const f32x4*)(row + e);
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = e + j < n ? row[e + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += v[j];
    }
    float s[CC];
    if (CC == 4) {
#pragma unroll
        for (int ch = 0; ch < CC; ++ch) s[ch] = a[ch];
    } else if (CC == 2) {
        s[0] = a[0] + a[2];
        s[CC - 1] = a[1] + a[3];
    } else {
        s[0] = (a[0] + a[1]) + (a[2] + a[3]);
    }
#pragma unroll
    for (int ch = 0; ch < CC; ++ch)
        for (int off = 32; off > 0; off >>= 1) s[ch] += __shfl_xor(s[ch], off);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int ch = 0; ch < CC; ++ch) wave_sum[threadIdx.x >> 6][ch] = s[ch];
    }
    __syncthreads();
    if (threadIdx.x < CC) {
        const int ch = threadIdx.x;
        partial[((long long)b * chunks + c) * CC + ch] = (wave_sum[0][ch] + wave_sum[1][ch]) + (wave_sum[2][ch] + wave_sum[3][ch]);
    }
}

__device__ __forceinline__ unsigned gm_field(u64 kb, int j) { return wa_field(kb, GM_FIELD + (u64)j); }

// Frequency mask d of a clip: (f0, w); needs Wa > 0.
__device__ __forceinline__ void gm_freq(u64 kb, const CpcGridMask& cfg, int H, int d, int& f0, int& w) {
    w = wa_int(gm_field(kb, 2 * d), 0, min(cfg.freq_max, H));
    f0 = wa_int(gm_field(kb, 2 * d + 1), 0, H - w);
}
// Time mask d of a clip: (t0, w); needs Wa > 0.
__device__ __forceinline__ void gm_time(u64 kb, const CpcGridMask& cfg, int Wa, int d, int& t0, int& w) {
    w = wa_int(gm_field(kb, 16 + 2 * d), 0, cfg.time_cap);
    t0 = wa_int(gm_field(kb, 17 + 2 * d), 0, Wa - w);
}

// What one clip drew: the same in every lane of the clip's workgroups; (0, 0) where nothing is drawn.
struct GridSpans {
    int f0[8], fw[8], t0[8], tw[8];
};
__device__ __forceinline__ void gm_draw(GridSpans& s, u64 kb, const CpcGridMask& cfg, int H, int Wa) {
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        s.f0[d] = s.fw[d] = s.t0[d] = s.tw[d] = 0;
        if (Wa > 0 && d < cfg.freq_count) gm_freq(kb, cfg, H, d, s.f0[d], s.fw[d]);
        if (Wa > 0 && d < cfg.time_count) gm_time(kb, cfg, Wa, d, s.t0[d], s.tw[d]);
    }
}

// The fill value of channel ch < Cc of clip b.  Mode 2: the sum of the clip's partials of that channel in index order, over float(W H).
// fill[j] for the four positions of a piece (position j holds channel j % Cc).  Called by whole waves in uniform control flow: lane l
// loads partial base + l of a block of 64 for every channel at once (one round trip per block instead of one per partial), and the chain
// takes them lane by lane — a chain of scalar loads cost 20 us of a 36 us in-place launch at 79 chunks ("Grid masking").
__device__ __forceinline__ void gm_fill(float (&fill)[4], const CpcGridMask& cfg, const float* __restrict__ partial, int b, int chunks,
                                        int Cc, float cells) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (cfg.fill_mode == 1) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) s[ch] = cfg.fill_value;
    } else if (cfg.fill_mode == 2) {
        const float* pr = partial + (long long)b * chunks * Cc;
        const int lane = threadIdx.x & 63;
        for (int base = 0; base < chunks; base += 64) {
            const int m = min(64, chunks - base);
            float v[4];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) v[ch] = ch < Cc && lane < m ? pr[(long long)(base + lane) * Cc + ch] : 0.f;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                if (ch >= Cc) continue;
                for (int i = 0; i < m; ++i)          // (the first addition, to 0, is exact)
                    s[ch] += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[ch]), i));
            }
        }
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) s[ch] = s[ch] / cells;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) fill[j] = s[j];
    if (Cc == 1) fill[1] = fill[0];
    if (Cc <= 2) {
        fill[2] = fill[0];
        fill[3] = fill[1];
    }
}

// spans_out[b][32] and fill_out[b][4] of one clip, by one thread.
__device__ __forceinline__ void gm_report(int* __restrict__ spans_out, float* __restrict__ fill_out, int b, const GridSpans& s,
                                          const float (&fill)[4], int Cc) {
    if (spans_out) {
        int* so = spans_out + 32ll * b;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            so[2 * d] = s.f0[d]; so[2 * d + 1] = s.fw[d];
            so[16 + 2 * d] = s.t0[d]; so[17 + 2 * d] = s.tw[d];
        }
    }
    if (fill_out) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) fill_out[4ll * b + ch] = ch < Cc ? fill[ch] : 0.f;
    }
}

// The copy form.  Workgroup (blockIdx.x, blockIdx.y): elements [8192 blockIdx.x, +8192) of clip blockIdx.y, a lane GM_COPY_ITERS pieces
// of 4 consecutive elements, 1024 elements apart.  A piece holds 4 / CC cells of one or two frames.
template <int CC>
__global__ __launch_bounds__(GM_THREADS) void grid_mask_copy_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                    const float* __restrict__ partial, int* __restrict__ spans_out,
                                                                    float* __restrict__ fill_out, int W, int H, unsigned n, long long ldbx,
                                                                    long long ldby, CpcGridMask cfg, int chunks, int vec_x, int vec_y) {
    const int b = blockIdx.y, Wa = W - cfg.protect_last;
    const u64 kb = wa_key(cfg.seed, cfg.step, cfg.clip_offset, b);
    GridSpans s;
    gm_draw(s, kb, cfg, H, Wa);
    const float* xr = x + (long long)b * ldbx;
    float* yr = y + (long long)b * ldby;
    float fill[4];
    gm_fill(fill, cfg, partial, b, chunks, CC, (float)W * (float)H);
    if ((spans_out || fill_out) && blockIdx.x == 0 && threadIdx.x == 0) gm_report(spans_out, fill_out, b, s, fill, CC);

    // (one piece at a time: with all eight loads of a lane issued in front of the first store the launch ran at 79 us instead of 71)
#pragma unroll
    for (int it = 0; it < GM_COPY_ITERS; ++it) {
        const unsigned e = 4u * (unsigned)(((int)blockIdx.x * GM_COPY_ITERS + it) * GM_THREADS + (int)threadIdx.x);
        if (e >= n) continue;
        const bool whole = e + 3u < n;
        float v[4];
        if (vec_x && whole) {
            const f32x4 q = *(const f32x4*)(xr + e);
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = e + j < n ? xr[e + j] : 0.f;
        }
        const unsigned cell = e / CC;
        int t = (int)(cell / (unsigned)H), h = (int)(cell - (unsigned)t * (unsigned)H);
#pragma unroll
        for (int q = 0; q < 4 / CC; ++q) {          // (cells behind the clip's last are computed on and never stored)
            bool hit = false;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                hit = hit || (unsigned)(t - s.t0[d]) < (unsigned)s.tw[d];          // the time spans lie inside [0, Wa)
                hit = hit || (t < Wa && (unsigned)(h - s.f0[d]) < (unsigned)s.fw[d]);
            }
#pragma unroll
            for (int j = q * CC; j < (q + 1) * CC; ++j) v[j] = hit ? fill[j] : v[j];
            if (++h == H) { h = 0; ++t; }
        }
        if (vec_y && whole) {
            *(f32x4*)(yr + e) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e + j < n) yr[e + j] = v[j];
        }
    }
}

// The in-place form: launched over the mask rectangles, it stores the fill into the masked cells and loads no grid element.
// Workgroup (blockIdx.x, r = blockIdx.y, b = blockIdx.z): rectangle r of clip b — frequency mask r for r < freq_count, else time mask
// r - freq_count — and of it the pieces [1024 blockIdx.x, +1024).  A rectangle is `rows` runs of R consecutive elements, `stride`
// elements apart, the first at s0: Wa runs of w Cc elements for a frequency mask, one run of w H Cc elements for a time mask.  A run
// is covered by the pieces of 4 elements that start at multiples of 4 from the clip's start (at most (R + 6) / 4 of them): a piece
// inside the run is one 16-byte store where the clip starts allow it, the elements of any other piece that lie inside the run are
// stored one by one.  Overlapping masks store the same value twice.  Workgroup (0, 0, b) also reports the clip's spans and fill.
__global__ __launch_bounds__(GM_THREADS) void grid_mask_rect_kernel(float* __restrict__ y, const float* __restrict__ partial,
                                                                    int* __restrict__ spans_out, float* __restrict__ fill_out, int W, int H,
                                                                    int Cc, long long ldb, CpcGridMask cfg, int chunks, int vec) {
    const int b = blockIdx.z, r = blockIdx.y, Wa = W - cfg.protect_last;
    const u64 kb = wa_key(cfg.seed, cfg.step, cfg.clip_offset, b);
    float fill[4];
    if ((spans_out || fill_out) && blockIdx.x == 0 && r == 0) {
        GridSpans s;
        gm_draw(s, kb, cfg, H, Wa);
        gm_fill(fill, cfg, partial, b, chunks, Cc, (float)W * (float)H);
        if (threadIdx.x == 0) gm_report(spans_out, fill_out, b, s, fill, Cc);
    }
    if (Wa == 0 || r >= cfg.freq_count + cfg.time_count) return;

    unsigned rows, stride, s0, R;
    if (r < cfg.freq_count) {
        int f0, w;
        gm_freq(kb, cfg, H, r, f0, w);
        rows = (unsigned)Wa; stride = (unsigned)(H * Cc); s0 = (unsigned)(f0 * Cc); R = (unsigned)(w * Cc);
    } else {
        int t0, w;
        gm_time(kb, cfg, Wa, r - cfg.freq_count, t0, w);
        rows = 1u; stride = 0u; s0 = (unsigned)t0 * (unsigned)(H * Cc); R = (unsigned)w * (unsigned)(H * Cc);
    }
    if (R == 0u) return;
    const unsigned per_row = (R + 6u) / 4u, total = rows * per_row;          // (total <= W H Cc: it fits)
    if (blockIdx.x * (unsigned)(GM_RECT_ITERS * GM_THREADS) >= total) return;          // behind this clip's own rectangle
    gm_fill(fill, cfg, partial, b, chunks, Cc, (float)W * (float)H);
    float* yr = y + (long long)b * ldb;
#pragma unroll
    for (int it = 0; it < GM_RECT_ITERS; ++it) {
        const unsigned q = (unsigned)(((int)blockIdx.x * GM_RECT_ITERS + it) * GM_THREADS + (int)threadIdx.x);
        if (q >= total) continue;
        const unsigned row = q / per_row, k = q - row * per_row;
        const unsigned lo = row * stride + s0, hi = lo + R;          // the run [lo, hi) of the clip
        const unsigned e = 4u * (lo / 4u + k);
        if (e >= hi) continue;
        if (vec && e >= lo && e + 4u <= hi) {
            *(f32x4*)(yr + e) = f32x4{fill[0], fill[1], fill[2], fill[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e + j >= lo && e + j < hi) yr[e + j] = fill[j];
        }
    }
}

}  // namespace

int grid_sum_chunks(int n) { return n < 1 ? 0 : (int)(((long long)n + GS_CHUNK - 1) / GS_CHUNK); }

int launch_grid_sum(const float* x, float* partial, int B, int n, long long ldb, int Cc, hipStream_t stream) {
    const int chunks = grid_sum_chunks(n);
    const dim3 grid(chunks, B), block(GM_THREADS);
    const bool vec = aligned16(x) && ldb % 4 == 0;
#define GS_LAUNCH(CC)                                                                                              \
    do {                                                                                                           \
        if (vec) grid_sum_kernel<CC, true><<<grid, block, 0, stream>>>(x, partial, ldb, (unsigned)n, chunks);      \
        else grid_sum_kernel<CC, false><<<grid, block, 0, stream>>>(x, partial, ldb, (unsigned)n, chunks);         \
    } while (0)
    if (Cc == 1) GS_LAUNCH(1);
    else if (Cc == 2) GS_LAUNCH(2);
    else GS_LAUNCH(4);
#undef GS_LAUNCH
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_grid_mask(const float* x, float* y, const float* partial, int* spans_out, float* fill_out, int B, int W, int H, int Cc,
                     long long ldbx, long long ldby, const cpc_grid_mask_cfg* cfg, hipStream_t stream) {
    const long long n = (long long)W * H * Cc;
    const int chunks = grid_sum_chunks((int)n), Wa = W - cfg->protect_last;
    const dim3 block(GM_THREADS);
    if (x != y) {
        const dim3 grid((unsigned)((n + 4ll * GM_THREADS * GM_COPY_ITERS - 1) / (4ll * GM_THREADS * GM_COPY_ITERS)), B);
        const int vec_x = aligned16(x) && ldbx % 4 == 0, vec_y = aligned16(y) && ldby % 4 == 0;
#define GM_LAUNCH(CC)                                                                                                                  \
    grid_mask_copy_kernel<CC><<<grid, block, 0, stream>>>(x, y, partial, spans_out, fill_out, W, H, (unsigned)n, ldbx, ldby, *cfg, chunks, \
                                                          vec_x, vec_y)
        if (Cc == 1) GM_LAUNCH(1);
        else if (Cc == 2) GM_LAUNCH(2);
        else GM_LAUNCH(4);
#undef GM_LAUNCH
        CPC_CHECK_LAUNCH();
        return CPC_OK;
    }
    // in place: the widest rectangle any clip can draw sizes the grid; workgroups behind a clip's own rectangle leave at once
    int rects = Wa > 0 ? cfg->freq_count + cfg->time_count : 0;
    long long pieces = 0;
    if (Wa > 0 && cfg->freq_count > 0) pieces = (long long)Wa * (((long long)(cfg->freq_max < H ? cfg->freq_max : H) * Cc + 6) / 4);
    if (Wa > 0 && cfg->time_count > 0) {
        const long long p = ((long long)cfg->time_cap * H * Cc + 6) / 4;
        pieces = p > pieces ? p : pieces;
    }
    if (rects == 0) {
        if (!spans_out && !fill_out) return CPC_OK;          // the identity, and nothing to report
        rects = 1;
    }
    const long long per_wg = (long long)GM_THREADS * GM_RECT_ITERS;
    const long long tiles = pieces < 1 ? 1 : (pieces + per_wg - 1) / per_wg;
    const dim3 grid((unsigned)tiles, rects, B);
    grid_mask_rect_kernel<<<grid, block, 0, stream>>>(y, partial, spans_out, fill_out, W, H, Cc, ldby, *cfg, chunks,
                                                      aligned16(y) && ldby % 4 == 0);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
