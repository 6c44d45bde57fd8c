// Log-mel front end (mel_spectrogram.py; not in the reference): what follows the framed DFT GEMM.
//   power |X|^2 -> mel bands (one f32 fma chain per band, ascending bins) -> scaling * log(. + log_offset) -> optional delta channel
// spec f32 [B][Tn][lds], (re, im) interleaved per bin, as cpc_gemm_nt leaves it.   out f32 [B][W][n_mels][Cc], channels-last:
// (W, Cc) = (Tn - 1, 2) with delta, (Tn, 1) without -- the buffer ScalogramCPCEngine reads in place.
#include "cpc_common.h"
#include "cpc_kernels.h"
#include <algorithm>

namespace {

constexpr int MEL_THREADS = 256;
constexpr int MEL_BANDS_PER_LANE = 4;          // n_mels <= 1024
constexpr int MEL_PASSES = 4;                  // a workgroup covers MEL_PASSES * FR consecutive spectrum frames of one clip
constexpr int MEL_LDS_FLOATS = 16384 - 16;     // 64 KB less the static LDS below: power rows of a pass + the staged weights

// acc[f] = fmaf(w[k], p[k][f], acc[f]) over k = k0 .. k1 - 1 ascending, for the FR frames of a pass at once (p is [bin][FR] in LDS:
// one 16-byte read per four frames).  Inlined once with the weights in LDS and once with them in global memory.
template <int FR>
__device__ __forceinline__ void mel_band_chain(const float* __restrict__ w, const float* __restrict__ p, int k0, int k1, float (&acc)[FR]) {
#pragma unroll 2
    for (int k = k0; k < k1; ++k) {
        const float wk = w[k];
        float pv[FR];
        if constexpr (FR >= 4) {
#pragma unroll
            for (int j = 0; j < FR / 4; ++j) {
                const float4 v = ((const float4*)(p + (size_t)k * FR))[j];
                pv[4 * j] = v.x; pv[4 * j + 1] = v.y; pv[4 * j + 2] = v.z; pv[4 * j + 3] = v.w;
            }
        } else {
            const float2 v = *(const float2*)(p + (size_t)k * FR);
            pv[0] = v.x; pv[1] = v.y;
        }
#pragma unroll
        for (int f = 0; f < FR; ++f) acc[f] = fmaf(wk, pv[f], acc[f]);
    }
}

// One workgroup = one clip b and one run of `span` = MEL_PASSES * FR spectrum frames [t0, t1).  A pass stages the powers of FR frames
// in LDS as [bin][FR]: thread k reads bin k of the FR rows (float2 per lane, a wave reads 512 contiguous bytes of each row; every
// spectrum row is read once) and writes FR contiguous floats.  Then lane `tid` owns bands tid, tid + 256, ...: one pass over the
// band's bins serves all FR frames.  The weight table is copied to LDS once per workgroup when it fits there (w_cap floats: a bank of
// triangles has at most 2 n_freq weights), and read from global memory otherwise.  With delta a run writes the span - 1 output
// frames t0 .. t1 - 2 and the next run starts at t1 - 1: one frame of overlap per run, and the log of a frame is carried in a
// register to the next frame (`carry`), not recomputed.  Every (frame, band) value is one chain in one order whatever FR, the grid
// and the place of the weights are: the results do not depend on any of them.
template <int FR>
__global__ __launch_bounds__(MEL_THREADS) void mel_pointwise_kernel(const float* __restrict__ spec, long long lds,
                                                                     const int* __restrict__ band_lo, const int* __restrict__ band_n,
                                                                     const int* __restrict__ band_off, const float* __restrict__ band_w,
                                                                     float* __restrict__ out, int Tn, int n_freq, int n_mels, int delta,
                                                                     int take_log, float log_offset, float scaling, float delta_scaling,
                                                                     int runs, int w_cap) {
    extern __shared__ __align__(16) float mel_smem[];          // power [n_freq][FR], then w_cap weights
    __shared__ int wave_end[MEL_THREADS / 64];
    float* mel_power = mel_smem;
    float* w_lds = mel_smem + (size_t)FR * n_freq;
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)runs), run = (int)(blockIdx.x % (unsigned)runs);
    const int span = MEL_PASSES * FR;
    const int t0 = run * (span - delta);
    const int t1 = min(Tn, t0 + span);
    const int W = Tn - delta;
    const float* clip = spec + (long long)b * Tn * lds;
    float* oclip = out + (long long)b * W * n_mels * (delta ? 2 : 1);

    // where the weight table ends (w_cap + 1: beyond what LDS holds, or a table with a negative entry), the largest over the workgroup
    int end = 0;
    for (int m = tid; m < n_mels; m += MEL_THREADS) {
        const int off = band_off[m], n = band_n[m];
        const long long e = (long long)off + max(n, 0);
        end = max(end, (off < 0 || e > w_cap) ? w_cap + 1 : (int)e);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) end = max(end, __shfl_xor(end, o));
    if ((tid & 63) == 0) wave_end[tid >> 6] = end;
    __syncthreads();
    end = max(max(wave_end[0], wave_end[1]), max(wave_end[2], wave_end[3]));
    const bool staged = end <= w_cap;
    if (staged)
        for (int i = tid; i < end; i += MEL_THREADS) w_lds[i] = band_w[i];

    float carry[MEL_BANDS_PER_LANE] = {0.f, 0.f, 0.f, 0.f};
    for (int s = t0; s < t1; s += FR) {
        const int nf = min(FR, t1 - s);
        __syncthreads();                                         // the previous pass has read its rows
        for (int k = tid; k < n_freq; k += MEL_THREADS) {
            float pv[FR];
#pragma unroll
            for (int f = 0; f < FR; ++f) {                       // (rows behind the run: the last row again, computed and not stored)
                const float2 z = ((const float2*)(clip + (long long)min(s + f, t1 - 1) * lds))[k];
                pv[f] = __fadd_rn(__fmul_rn(z.x, z.x), __fmul_rn(z.y, z.y));      // three roundings, never contracted
            }
            if constexpr (FR >= 4) {
#pragma unroll
                for (int j = 0; j < FR / 4; ++j)
                    ((float4*)(mel_power + (size_t)k * FR))[j] = make_float4(pv[4 * j], pv[4 * j + 1], pv[4 * j + 2], pv[4 * j + 3]);
            } else {
                *(float2*)(mel_power + (size_t)k * FR) = make_float2(pv[0], pv[1]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MEL_BANDS_PER_LANE; ++i) {
            const int m = tid + i * MEL_THREADS;
            if (m >= n_mels) continue;
            // the band's bin range, clamped to the spectrum row (a wrong table cannot read outside it)
            const int lo = band_lo[m];
            const int k0 = min(max(lo, 0), n_freq);
            const int k1 = (int)min(max((long long)lo + band_n[m], (long long)k0), (long long)n_freq);
            const long long shift = (long long)band_off[m] - lo;          // weight of bin k: index shift + k
            float acc[FR];
#pragma unroll
            for (int f = 0; f < FR; ++f) acc[f] = 0.f;
            if (staged) mel_band_chain<FR>(w_lds + shift, mel_power, k0, k1, acc);
            else mel_band_chain<FR>(band_w + shift, mel_power, k0, k1, acc);
#pragma unroll
            for (int f = 0; f < FR; ++f) {
                if (f >= nf) continue;
                const int t = s + f;
                if (!take_log) {
                    oclip[(long long)t * n_mels + m] = acc[f];
                    continue;
                }
                const float l = logf(acc[f] + log_offset);
                if (!delta)
                    oclip[(long long)t * n_mels + m] = scaling * l;
                else if (t > t0)
                    *(float2*)(oclip + ((long long)(t - 1) * n_mels + m) * 2) = make_float2(scaling * l, delta_scaling * (l - carry[i]));
                carry[i] = l;
            }
        }
    }
}

}  // namespace

// Arguments are checked by cpc_mel_pointwise (cpc_abi.hip).  Frames per pass by the LDS a pass needs: 8 up to n_fft = 2048, 4 up to
// 4096, 2 above; room for 2 n_freq staged weights behind the powers (fewer at n_freq = 4097: 64 KB in all).
int launch_mel_pointwise(const float* spec, long long lds, const int* band_lo, const int* band_n, const int* band_off, const float* band_w,
                         float* out, int B, int Tn, int n_freq, int n_mels, int delta, int take_log, float log_offset, float scaling,
                         float delta_scaling, hipStream_t stream) {
    const int fr = n_freq <= 1025 ? 8 : (n_freq <= 2049 ? 4 : 2);
    const int span = MEL_PASSES * fr;
    const int W = Tn - delta;
    const int runs = (W + (span - delta) - 1) / (span - delta);
    const long long blocks = (long long)B * runs;
    if (blocks > 0x7fffffffLL) return CPC_EINVAL;
    const int w_cap = std::min(2 * n_freq, MEL_LDS_FLOATS - fr * n_freq);
    const size_t shmem = (size_t)(fr * n_freq + w_cap) * sizeof(float);
#define MEL_LAUNCH(FR)                                                                                                              \
    hipLaunchKernelGGL(mel_pointwise_kernel<FR>, dim3((unsigned)blocks), dim3(MEL_THREADS), shmem, stream, spec, lds, band_lo, band_n, \
                       band_off, band_w, out, Tn, n_freq, n_mels, delta, take_log, log_offset, scaling, delta_scaling, runs, w_cap)
    if (fr == 8) MEL_LAUNCH(8);
    else if (fr == 4) MEL_LAUNCH(4);
    else MEL_LAUNCH(2);
#undef MEL_LAUNCH
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
