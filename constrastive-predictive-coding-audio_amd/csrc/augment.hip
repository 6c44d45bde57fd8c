// Waveform augmentation in the time domain (include/cpc_hip.h, cpc_wave_power / cpc_wave_augment; DESIGN.md, "Waveform
// augmentation"): speed change, time drop, additive noise, gain and polarity on the first protect_from samples of every clip.
// Memory-bound by design: the batch is read once by the power pass and once by the apply pass, and written once.  Every random number
// is a pure function of (seed, step, clip, field or sample index) with the arithmetic of drop_hash (attn.hip) and of the sampled
// negatives (nce.hip), so a launch has no state, the host can restate every draw, and a shard of a batch draws what the whole batch
// draws for its clips.  No atomics, no LDS beyond the four wave sums of the power pass, every sum in one fixed order.
#include <cmath>
#include "cpc_common.h"
#include "cpc_draws.h"
#include "cpc_kernels.h"
#include "../../include/cpc_hip.h"

namespace {

constexpr int WA_THREADS = 256;
constexpr int WP_CHUNK = 4096;                        // samples per partial sum of the power pass: 256 threads x 4 pieces x 4 floats
// Pieces of 4 outputs a lane of the apply pass writes, 1024 samples apart.  A lane's share of the per-clip draws (a dozen 64-bit
// hashes, two exp2f, a square root and a division, the same in every lane) costs more than the per-sample work of one piece: at one
// piece per lane the pass ran at 22 - 28 us for 256 x 20480 samples, DESIGN.md has the figures per count.
constexpr int WA_ITERS = 4;
constexpr int WA_TILE = WA_THREADS * 4 * WA_ITERS;    // outputs per workgroup of the apply pass
constexpr int WA_NOISE_FIELD = 32;                    // per-sample hashes start behind the per-clip fields
constexpr float WA_DB = 0.16609640474436813f;         // log2(10) / 20
constexpr float WA_G = 2.642899791822139e-05f;        // sqrt(3) / 65536

// partial[b][c] = sum of squares of x[b][4096 c .. min(4096 (c + 1), n)).  Thread t: one fma chain over the elements
// 4 (256 p + t) + j (p outer, j inner; zeros behind n leave the chain's value as it is), the butterfly, the four waves.  VEC only
// changes how the same elements are loaded.
template <bool VEC>
__global__ __launch_bounds__(WA_THREADS) void wave_power_kernel(const float* __restrict__ x, float* __restrict__ partial, long long ldx,
                                                                int n, int chunks) {
    __shared__ float wave_sum[WA_THREADS / 64];
    const int c = blockIdx.x, b = blockIdx.y;
    const float* row = x + (long long)b * ldx;
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int e = c * WP_CHUNK + 4 * (p * WA_THREADS + (int)threadIdx.x);
        float v[4];
        if (VEC && e + 3 < n) {
            const f32x4 q = *(const f32x4*)(row + e);
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = e + j < n ? row[e + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(v[j], v[j], s);
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[(long long)b * chunks + c] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// x[i], 0 outside [0, L).  The load itself is unconditional, from the index clamped into the row (L >= 1), and the zero is a select
// behind it: a load under a condition compiles to a branch per tap (214 branches in the speed-on kernels against 122 this way).
__device__ __forceinline__ float wa_tap(const float* row, int i, int L) {
    const float v = row[min(max(i, 0), L - 1)];
    return (unsigned)i < (unsigned)L ? v : 0.f;
}

// Output n < a of a clip resampled at the rate q (Q16), anchored at a.
__device__ __forceinline__ float wa_resample(const float* row, int L, int a, int q, int n) {
    const long long pos = (long long)a * 65536 - (long long)(a - n) * q;
    const int i = (int)(pos >> 16);
    const float t = (float)(int)(pos & 0xFFFF) * 0x1p-16f, u = 1.f - t;          // both exact
    const float wm = -0.5f * ((t * u) * u);
    const float w0 = 0.5f * (u * fmaf(t, fmaf(-3.f, t, 2.f), 2.f));
    const float w1 = 0.5f * (t * fmaf(t, fmaf(-3.f, t, 4.f), 1.f));
    const float w2 = -0.5f * ((t * t) * u);
    float v = wm * wa_tap(row, i - 1, L);
    v = fmaf(w0, wa_tap(row, i, L), v);
    v = fmaf(w1, wa_tap(row, i + 1, L), v);
    return fmaf(w2, wa_tap(row, i + 2, L), v);
}

// What one clip drew: the same in every lane of the clip's workgroups.
struct WaveClip {
    u64 kb;
    int a, q;
    int ds[8], dl[8];
    float sigma, gain;
    bool dropping, scale, flip;
};

// 4 consecutive outputs n0 .. n0 + 3 of one clip.
template <bool SPEED, bool NOISE>
__device__ __forceinline__ void wa_piece(const WaveClip& c, const float* __restrict__ xr, float* __restrict__ yr, int n0, int L, int vec_x,
                                         int vec_y) {
    const int a = c.a;
    const bool whole = n0 + 3 < L;
    float v[4];
    if (!SPEED || n0 >= a) {          // the stored samples themselves: every speed-off output, and the protected tail
        if (vec_x && whole) {
            const f32x4 p = *(const f32x4*)(xr + n0);
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = n0 + j < L ? xr[n0 + j] : 0.f;
        }
    } else {
        float tail[4] = {0.f, 0.f, 0.f, 0.f};
        if (n0 + 3 >= a) {            // the one piece of a clip that straddles a
#pragma unroll
            for (int j = 0; j < 4; ++j) tail[j] = wa_tap(xr, n0 + j, L);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float r = wa_resample(xr, L, a, c.q, n0 + j);
            v[j] = n0 + j < a ? r : tail[j];
        }
    }
    if (n0 < a) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + j;
            if (n >= a) continue;
            float w = v[j];
            if (c.dropping) {
                bool hit = false;
#pragma unroll
                for (int d = 0; d < 8; ++d) hit = hit || (unsigned)(n - c.ds[d]) < (unsigned)c.dl[d];
                if (hit) w = 0.0f;
            }
            if (NOISE) {
                const u64 h = wa_mix(c.kb + WA_IDX * (u64)(WA_NOISE_FIELD + n));
                const int s = (int)((unsigned)h & 0xFFFFu) + (int)((unsigned)(h >> 16) & 0xFFFFu) + (int)((unsigned)(h >> 32) & 0xFFFFu) +
                              (int)(unsigned)(h >> 48);
                w = fmaf(c.sigma, (float)(s - 131070) * WA_G, w);
            }
            if (c.scale) w = w * c.gain;
            else if (c.flip) w = -w;
            v[j] = w;
        }
    }
    if (vec_y && whole) {
        *(f32x4*)(yr + n0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n0 + j < L) yr[n0 + j] = v[j];
    }
}

// Workgroup (blockIdx.x, blockIdx.y): outputs [WA_TILE blockIdx.x, +WA_TILE) of clip blockIdx.y, a lane WA_ITERS pieces of 4.
template <bool SPEED, bool NOISE>
__global__ __launch_bounds__(WA_THREADS) void wave_augment_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                  const float* __restrict__ partial, float* __restrict__ params_out, int L,
                                                                  long long ldx, long long ldy, CpcWaveAugment cfg, int vec_x, int vec_y) {
    const int b = blockIdx.y, a = cfg.protect_from;
    const bool live = a > 0;
    WaveClip c;
    c.kb = wa_key(cfg.seed, cfg.step, cfg.clip_offset, b);
    c.a = a;
    c.q = 65536;
    if (SPEED && live) c.q = wa_int(wa_field(c.kb, 1), cfg.q_lo, cfg.q_hi);
    c.dropping = live && cfg.drop_count > 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        c.ds[d] = 0;
        c.dl[d] = 0;
        if (c.dropping && d < cfg.drop_count) {
            c.dl[d] = wa_int(wa_field(c.kb, 8 + 2 * d), 1, min(cfg.drop_max_len, a));
            c.ds[d] = wa_int(wa_field(c.kb, 9 + 2 * d), 0, a - c.dl[d]);
        }
    }
    float power = 0.f;
    c.sigma = 0.f;
    if (NOISE && live) {
        const int chunks = (a + WP_CHUNK - 1) / WP_CHUNK;
        const float* pr = partial + (long long)b * chunks;
        float s = pr[0];
        for (int k = 1; k < chunks; ++k) s += pr[k];
        power = s / (float)a;
        const float snr_db = wa_real(wa_field(c.kb, 2), cfg.snr_lo, cfg.snr_hi);
        c.sigma = sqrtf(power) * exp2f(-snr_db * WA_DB);
    }
    c.scale = live && cfg.gain_on != 0;
    c.flip = live && (u64)wa_field(c.kb, 4) < cfg.polarity_threshold;
    c.gain = 1.f;
    if (c.scale) c.gain = exp2f(wa_real(wa_field(c.kb, 3), cfg.gain_lo_db, cfg.gain_hi_db) * WA_DB);
    if (c.flip) c.gain = -c.gain;
    if (params_out && blockIdx.x == 0 && threadIdx.x == 0) {
        float* po = params_out + 8ll * b;
        po[0] = (float)c.q; po[1] = c.sigma; po[2] = c.gain; po[3] = power;
        po[4] = (float)c.ds[0]; po[5] = (float)c.dl[0]; po[6] = (float)c.ds[1]; po[7] = (float)c.dl[1];
    }

    const float* xr = x + (long long)b * ldx;
    float* yr = y + (long long)b * ldy;
#pragma unroll
    for (int it = 0; it < WA_ITERS; ++it) {
        const int n0 = 4 * (((int)blockIdx.x * WA_ITERS + it) * WA_THREADS + (int)threadIdx.x);
        if (n0 < L) wa_piece<SPEED, NOISE>(c, xr, yr, n0, L, vec_x, vec_y);
    }
}

}  // namespace

int wave_power_chunks(int n) { return n < 1 ? 0 : (n + WP_CHUNK - 1) / WP_CHUNK; }

int launch_wave_power(const float* x, float* partial, int B, int L, long long ldx, int n, hipStream_t stream) {
    const int chunks = wave_power_chunks(n);
    const dim3 grid(chunks, B), block(WA_THREADS);
    if (aligned16(x) && ldx % 4 == 0)
        wave_power_kernel<true><<<grid, block, 0, stream>>>(x, partial, ldx, n, chunks);
    else
        wave_power_kernel<false><<<grid, block, 0, stream>>>(x, partial, ldx, n, chunks);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_wave_augment(const float* x, float* y, const float* partial, float* params_out, int B, int L, long long ldx, long long ldy,
                        const cpc_wave_augment_cfg* cfg, hipStream_t stream) {
    const dim3 grid((L + WA_TILE - 1) / WA_TILE, B), block(WA_THREADS);
    const int vec_x = aligned16(x) && ldx % 4 == 0, vec_y = aligned16(y) && ldy % 4 == 0;
    const bool speed = !(cfg->q_lo == 65536 && cfg->q_hi == 65536), noise = cfg->noise_on != 0;
#define WA_LAUNCH(S, N) wave_augment_kernel<S, N><<<grid, block, 0, stream>>>(x, y, partial, params_out, L, ldx, ldy, *cfg, vec_x, vec_y)
    if (speed && noise) WA_LAUNCH(true, true);
    else if (speed) WA_LAUNCH(true, false);
    else if (noise) WA_LAUNCH(false, true);
    else WA_LAUNCH(false, false);
#undef WA_LAUNCH
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
