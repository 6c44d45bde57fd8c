// K-means over feature rows (include/cpc_hip.h, cpc_kmeans_assign / cpc_kmeans_update / cpc_kmeans_cnorm; DESIGN.md, "K-means units").
//   assign   per row the index of the smallest cnorm[k] - 2 x.c_k.  A workgroup owns 128 rows and walks the centres in chunks of 128
//            (or 64); rows and centres go through LDS as f32, 32 columns of D at a time, and the products are f32-input MFMAs
//            (32x32x2: exact f32, one rounding per product, no wider accumulation).  Centres sit on the MFMA's row index and x rows
//            on its column index, so a lane holds 16 centres of ONE x row per tile and the running (min, argmin) of that row stays
//            in its registers across chunks; the two lane halves of a row meet once, at the end.  The N x K products never leave
//            the registers.
//   update   a stable counting sort of the row indices by label (per-block histograms, a scan over (cluster, block), an in-block
//            stable rank), then per cluster sums over fixed-length pieces of its rows and a fold of the pieces in order.  Every
//            floating-point sum is f64 from the first addition and has an order fixed by (N, K, D); the only atomics are the
//            integer ones of the histogram.
#include <cmath>
#include "cpc_common.h"
#include "cpc_kernels.h"
#include "../../include/cpc_hip.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int KM_BM = 128;               // x rows of a workgroup
constexpr int KM_DK = 32;                // columns staged per pass
constexpr int KM_LD = KM_DK + 4;         // LDS row stride in floats: 16-byte reads of 8 consecutive rows cover the 32 banks once

__device__ __forceinline__ unsigned nonfinite_bit(float v) {
    return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
}

// ------------------------------------------------------------------------------------------------------------------ assign
// TA: 32-centre MFMA tiles per chunk (4: chunks of 128 centres, 2: chunks of 64).  Wave w owns x rows [32 w, +32) of the tile and all
// centres of the chunk.  Lane l = (j = l & 31, h = l >> 5): B operand x row j, A operand centre j of a tile; of a step of 8 columns it
// reads the 4 at 4 h as 16 bytes and MFMA e takes element e of both operands (the same k permutation on both sides).  Accumulator
// register r of tile ta is centre 32 ta + (r & 3) + 8 (r >> 2) + 4 h against x row j: ascending in r, so a strict < keeps the lowest
// index inside a lane.
template <typename T, int TA>
__global__ __launch_bounds__(256, 2) void kmeans_assign_kernel(const T* __restrict__ x, long long N, int D, long long ldx,
                                                            const float* __restrict__ centers, const float* __restrict__ cnorm, int K,
                                                            int* __restrict__ labels, float* __restrict__ dist) {
    constexpr int CH = Elem<T>::CH;
    constexpr int KC = 32 * TA;
    constexpr int XCPR = KM_DK / CH;                 // 16-byte pieces of a staged x row
    constexpr int XROWS = 256 / XCPR;                // x rows a pass of the workgroup stages
    constexpr int XPASS = KM_BM / XROWS;
    constexpr int CPASS = KC / 32;                   // (8 pieces per centre row, 32 rows a pass)
    __shared__ __attribute__((aligned(16))) float xs[KM_BM * KM_LD];
    __shared__ __attribute__((aligned(16))) float cs[KC * KM_LD];
    __shared__ float xn_s[KM_BM];
    __shared__ unsigned bad_s[KM_BM];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6, j = lane & 31, h = lane >> 5;
    const long long n0 = (long long)blockIdx.x * KM_BM;
    const int xrow = t / XCPR, xpc = t % XCPR, crow = t >> 3, cpc = t & 7;
    const int nd = D / KM_DK + (D % KM_DK ? 1 : 0);          // D is a multiple of 16: the last pass may hold 16 columns
    const int nkc = (K + KC - 1) / KC;

    uint4 xr[XPASS], cr[CPASS];
    float ss[XPASS];
    unsigned bad[XPASS];
#pragma unroll
    for (int p = 0; p < XPASS; ++p) { ss[p] = 0.f; bad[p] = 0u; }

    auto load_regs = [&](int kc, int d0) {
#pragma unroll
        for (int p = 0; p < XPASS; ++p) {
            const long long n = n0 + xrow + p * XROWS;
            const int d = d0 + xpc * CH;
            xr[p] = uint4{0u, 0u, 0u, 0u};
            if (n < N && d < D) xr[p] = *(const uint4*)(x + n * ldx + d);
        }
#pragma unroll
        for (int p = 0; p < CPASS; ++p) {
            const int k = kc + crow + 32 * p, d = d0 + cpc * 4;
            cr[p] = uint4{0u, 0u, 0u, 0u};
            if (k < K && d < D) cr[p] = *(const uint4*)(centers + (long long)k * D + d);
        }
    };
    auto store_regs = [&](bool first) {
#pragma unroll
        for (int p = 0; p < XPASS; ++p) {
            float v[CH];
            if constexpr (sizeof(T) == 4) {
                const f32x4 f = __builtin_bit_cast(f32x4, xr[p]);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = f[e];
            } else {
                const bf16x8 f = __builtin_bit_cast(bf16x8, xr[p]);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (float)f[e];
            }
            float* dst = xs + (xrow + p * XROWS) * KM_LD + xpc * CH;
#pragma unroll
            for (int e = 0; e < CH; e += 4) *(f32x4*)(dst + e) = f32x4{v[e], v[e + 1], v[e + 2], v[e + 3]};
            if (first) {
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    ss[p] = fmaf(v[e], v[e], ss[p]);
                    bad[p] |= nonfinite_bit(v[e]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < CPASS; ++p) *(uint4*)(cs + (crow + 32 * p) * KM_LD + cpc * 4) = cr[p];
    };

    f32x16 acc[TA];
    float best = INFINITY;
    int arg = 0;
    const float* bp = xs + (w * 32 + j) * KM_LD + 4 * h;
    const float* ap = cs + j * KM_LD + 4 * h;

    load_regs(0, 0);
    for (int ic = 0; ic < nkc; ++ic) {
        const int kc = ic * KC;
#pragma unroll
        for (int ta = 0; ta < TA; ++ta)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ta][r] = 0.f;
        for (int id = 0; id < nd; ++id) {
            store_regs(ic == 0);
            __syncthreads();
            if (id + 1 < nd) load_regs(kc, (id + 1) * KM_DK);
            else if (ic + 1 < nkc) load_regs(kc + KC, 0);
#pragma unroll
            for (int s = 0; s < KM_DK / 8; ++s) {
                const f32x4 b = *(const f32x4*)(bp + 8 * s);
#pragma unroll
                for (int ta = 0; ta < TA; ++ta) {
                    const f32x4 a = *(const f32x4*)(ap + ta * 32 * KM_LD + 8 * s);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[ta] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc[ta], 0, 0, 0);
                }
            }
            if (ic == 0 && id == nd - 1) {
                // |x|^2 and the non-finite flag of the staged rows: the XCPR neighbouring lanes of a row, as a symmetric tree
#pragma unroll
                for (int p = 0; p < XPASS; ++p) {
                    float s2 = ss[p];
                    unsigned bd = bad[p];
#pragma unroll
                    for (int m = 1; m < XCPR; m <<= 1) {
                        s2 += __shfl_xor(s2, m);
                        bd |= (unsigned)__shfl_xor((int)bd, m);
                    }
                    if (xpc == 0) {
                        xn_s[xrow + p * XROWS] = s2;
                        bad_s[xrow + p * XROWS] = bd;
                    }
                }
            }
            __syncthreads();
        }
        // the chunk's candidates of this lane, ascending in the centre index; padded centres are never compared
#pragma unroll
        for (int ta = 0; ta < TA; ++ta) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = kc + 32 * ta + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (k < K) {
                    const float v = fmaf(-2.f, acc[ta][r], cnorm[k]);
                    if (v < best) { best = v; arg = k; }
                }
            }
        }
    }
    // the two halves of a row: the smaller value, the lower index on a tie
    const float ob = __shfl_xor(best, 32);
    const int oa = __shfl_xor(arg, 32);
    if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    const long long n = n0 + w * 32 + j;
    if (h == 0 && n < N) {
        const bool isbad = bad_s[w * 32 + j] != 0u;
        labels[n] = isbad ? -1 : arg;
        if (dist) dist[n] = isbad ? NAN : fmaxf(best + xn_s[w * 32 + j], 0.f);
    }
}

// ------------------------------------------------------------------------------------------------------------------ update
struct KmPlan {
    long long RB, PL, PMAX, bytes;          // rows per sort block, rows per piece, most pieces
    int NB;                                 // sort blocks
    long long off_hist, off_ccount, off_cstart, off_pstart, off_perm, off_ipart, off_part;
};

long long km_up(long long v, long long m) { return (v + m - 1) / m * m; }

KmPlan km_plan(long long N, int K, int D) {
    KmPlan p;
    p.RB = km_up((N + 4095) / 4096, 1024);                  // at most 4096 sort blocks
    p.NB = (int)((N + p.RB - 1) / p.RB);
    p.PL = km_up((N + 16383) / 16384, 256);                 // at most 16384 + K pieces
    p.PMAX = (N + p.PL - 1) / p.PL + K;
    long long o = 0;
    p.off_hist = o;   o = km_up(o + 4ll * p.NB * K, 256);
    p.off_ccount = o; o = km_up(o + 4ll * K, 256);
    p.off_cstart = o; o = km_up(o + 4ll * (K + 1), 256);
    p.off_pstart = o; o = km_up(o + 4ll * (K + 1), 256);
    p.off_perm = o;   o = km_up(o + 4ll * N, 256);
    p.off_ipart = o;  o = km_up(o + 8ll * p.NB, 256);
    p.off_part = o;   o = km_up(o + 8ll * p.PMAX * D, 256);
    p.bytes = o;
    return p;
}

// the 256 values of a workgroup as a fixed tree
__device__ __forceinline__ double block_sum_256(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
#pragma unroll
    for (int m = 128; m > 0; m >>= 1) {
        __syncthreads();
        if (t < m) red[t] += red[t + m];
    }
    __syncthreads();
    return red[0];
}

// Sort block b = rows [b RB, + RB): the histogram of its valid labels, and the f64 sum of their distances.
__global__ __launch_bounds__(256) void km_hist_kernel(const int* __restrict__ labels, const float* __restrict__ dist, long long N,
                                                      int K, long long RB, int* __restrict__ hist, double* __restrict__ ipart) {
    __shared__ int hs[1024];
    __shared__ double red[256];
    const int t = threadIdx.x;
    for (int k = t; k < K; k += 256) hs[k] = 0;
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * RB, r1 = min(N, r0 + RB);
    double s = 0.0;
    for (long long r = r0 + t; r < r1; r += 256) {
        const int l = labels[r];
        if ((unsigned)l < (unsigned)K) {
            atomicAdd(&hs[l], 1);
            if (dist) s += (double)dist[r];
        }
    }
    __syncthreads();
    for (int k = t; k < K; k += 256) hist[(long long)blockIdx.x * K + k] = hs[k];
    const double tot = block_sum_256(s, red);
    if (t == 0) ipart[blockIdx.x] = tot;
}

// Cluster k = blockIdx.x (one wave): hist[b][k] becomes the number of rows with label k in the blocks before b; ccount[k] their total.
__global__ __launch_bounds__(64) void km_blockscan_kernel(int* __restrict__ hist, int NB, int K, int* __restrict__ ccount) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int S = (NB + 63) / 64, b0 = min(NB, lane * S), b1 = min(NB, b0 + S);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += hist[(long long)b * K + k];
    int incl = s;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_up(incl, m);
        if (lane >= m) incl += o;
    }
    int run = incl - s;
    for (int b = b0; b < b1; ++b) {
        const int c = hist[(long long)b * K + k];
        hist[(long long)b * K + k] = run;
        run += c;
    }
    if (lane == 63) ccount[k] = incl;
}

// One workgroup: cstart[k] = first sorted position of cluster k, pstart[k] = its first piece (ceil(count / PL) pieces each), both with
// the total at [K]; the distance sums of the sort blocks folded into *inertia.
__global__ __launch_bounds__(1024) void km_offsets_kernel(const int* __restrict__ ccount, int K, long long PL, int* __restrict__ cstart,
                                                          int* __restrict__ pstart, const double* __restrict__ ipart, int NB,
                                                          double* __restrict__ inertia) {
    __shared__ int sa[1024], sb[1024];
    __shared__ double red[1024];
    const int t = threadIdx.x;
    const int a = t < K ? ccount[t] : 0, q = (int)((a + PL - 1) / PL);
    sa[t] = a;
    sb[t] = q;
    __syncthreads();
    for (int m = 1; m < 1024; m <<= 1) {
        const int va = t >= m ? sa[t - m] : 0, vb = t >= m ? sb[t - m] : 0;
        __syncthreads();
        sa[t] += va;
        sb[t] += vb;
        __syncthreads();
    }
    if (t < K) {
        cstart[t] = sa[t] - a;
        pstart[t] = sb[t] - q;
        if (t == K - 1) {
            cstart[K] = sa[t];
            pstart[K] = sb[t];
        }
    }
    if (inertia) {
        double s = 0.0;
        for (int b = t; b < NB; b += 1024) s += ipart[b];
        red[t] = s;
        for (int m = 512; m > 0; m >>= 1) {
            __syncthreads();
            if (t < m) red[t] += red[t + m];
        }
        if (t == 0) *inertia = red[0];
    }
}

// Sort block b (one wave): its rows in ascending order, 64 at a time; a row's position is its cluster's start, plus the rows of the
// cluster in earlier blocks, plus those before it in this block.  perm[position] = row.
__global__ __launch_bounds__(64) void km_rank_kernel(const int* __restrict__ labels, long long N, int K, long long RB,
                                                     const int* __restrict__ rel, const int* __restrict__ cstart, int* __restrict__ perm) {
    __shared__ int cnt[1024];
    const int lane = threadIdx.x;
    for (int k = lane; k < K; k += 64) cnt[k] = cstart[k] + rel[(long long)blockIdx.x * K + k];
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * RB, r1 = min(N, r0 + RB);
    for (long long base = r0; base < r1; base += 64) {
        const long long r = base + lane;
        const int l = r < r1 ? labels[r] : -1;
        bool todo = (unsigned)l < (unsigned)K;
        int pos = -1;
        for (;;) {
            const unsigned long long rem = __ballot(todo);          // (uniform over the wave, which is the workgroup)
            if (!rem) break;
            const int leader = __ffsll((long long)rem) - 1;
            const int ll = __shfl(l, leader);
            const bool mine = todo && l == ll;
            const unsigned long long m = __ballot(mine);
            const int first = cnt[ll];
            __syncthreads();
            if (mine) {
                pos = first + __popcll(m & ((1ull << lane) - 1ull));
                todo = false;
            }
            if (lane == leader) cnt[ll] = first + __popcll(m);
            __syncthreads();
        }
        if (pos >= 0) perm[pos] = (int)r;
    }
}

// Piece p = blockIdx.x: rows [j PL, + PL) of the sorted rows of its cluster.  Thread (g, c): 16-byte piece c of the rows g, g + G, ...
// of the piece; the G groups are then added in order.  part[p][D] f64.
template <typename T>
__global__ __launch_bounds__(256) void km_segsum_kernel(const T* __restrict__ x, int D, long long ldx, int K, long long PL,
                                                        const int* __restrict__ perm, const int* __restrict__ cstart,
                                                        const int* __restrict__ pstart, double* __restrict__ part) {
    constexpr int CH = Elem<T>::CH;
    __shared__ double red[256 * CH];
    const int p = blockIdx.x, t = threadIdx.x;
    if (p >= pstart[K]) return;
    int lo = 0, hi = K;                       // the last k with pstart[k] <= p (clusters without rows have no piece)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pstart[mid] <= p) lo = mid; else hi = mid;
    }
    const int k = lo;
    const long long first = cstart[k] + (long long)(p - pstart[k]) * PL;
    const int cnt = (int)min(PL, (long long)cstart[k + 1] - first);
    const int CPR = D / CH, G = 256 / CPR, c = t % CPR, g = t / CPR;
    double s[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) s[e] = 0.0;
    if (g < G) {
        for (int i = g; i < cnt; i += G) {
            const long long row = perm[first + i];
            const uint4 raw = *(const uint4*)(x + row * ldx + c * CH);
            if constexpr (sizeof(T) == 4) {
                const f32x4 f = __builtin_bit_cast(f32x4, raw);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += (double)f[e];
            } else {
                const bf16x8 f = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
                for (int e = 0; e < 8; ++e) s[e] += (double)(float)f[e];
            }
        }
#pragma unroll
        for (int e = 0; e < CH; ++e) red[g * D + c * CH + e] = s[e];
    }
    __syncthreads();
    for (int d = t; d < D; d += 256) {
        double tot = 0.0;
        for (int gg = 0; gg < G; ++gg) tot += red[gg * D + d];
        part[(long long)p * D + d] = tot;
    }
}

__device__ __forceinline__ void km_write_norm(double sq, float* cnorm, int k, double* red) {
    const double tot = block_sum_256(sq, red);
    if (threadIdx.x == 0) cnorm[k] = (float)tot;
}

// Cluster k = blockIdx.x: its pieces added in order, the mean rounded once to f32; without rows the old centre, bit for bit.
__global__ __launch_bounds__(256) void km_fold_kernel(const double* __restrict__ part, const int* __restrict__ cstart,
                                                      const int* __restrict__ pstart, const float* centers_old, int D, float* centers_new,
                                                      float* __restrict__ cnorm, int* __restrict__ counts) {
    __shared__ double red[256];
    const int k = blockIdx.x, t = threadIdx.x;
    const int n = cstart[k + 1] - cstart[k], p0 = pstart[k], np = pstart[k + 1] - p0;
    double sq = 0.0;
    for (int d = t; d < D; d += 256) {
        float c;
        if (n > 0) {
            double tot = 0.0;
#pragma unroll 8
            for (int jp = 0; jp < np; ++jp) tot += part[(long long)(p0 + jp) * D + d];
            c = (float)(tot / (double)n);
        } else {
            c = centers_old[(long long)k * D + d];
        }
        centers_new[(long long)k * D + d] = c;
        sq += (double)c * (double)c;
    }
    km_write_norm(sq, cnorm, k, red);
    if (t == 0) counts[k] = n;
}

__global__ __launch_bounds__(256) void km_cnorm_kernel(const float* __restrict__ centers, int D, float* __restrict__ cnorm) {
    __shared__ double red[256];
    const int k = blockIdx.x;
    double sq = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) {
        const double c = (double)centers[(long long)k * D + d];
        sq += c * c;
    }
    km_write_norm(sq, cnorm, k, red);
}

}  // namespace

long long kmeans_scratch_bytes(long long N, int K, int D) { return km_plan(N, K, D).bytes; }

int launch_kmeans_assign(const void* x, int dtype, long long N, int D, long long ldx, const float* centers, const float* cnorm, int K,
                         int* labels, float* dist, hipStream_t stream) {
    const unsigned grid = (unsigned)((N + KM_BM - 1) / KM_BM);
    // chunks of 64 centres where they leave fewer padded columns than chunks of 128
    const bool narrow = (K + 63) / 64 * 64 < (K + 127) / 128 * 128;
#define ASSIGN(T, TA) kmeans_assign_kernel<T, TA><<<grid, 256, 0, stream>>>((const T*)x, N, D, ldx, centers, cnorm, K, labels, dist)
    if (dtype == CPC_DTYPE_BF16) { if (narrow) ASSIGN(bf16_t, 2); else ASSIGN(bf16_t, 4); }
    else { if (narrow) ASSIGN(float, 2); else ASSIGN(float, 4); }
#undef ASSIGN
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_kmeans_update(const void* x, int dtype, long long N, int D, long long ldx, const int* labels, const float* dist,
                         const float* centers_old, int K, void* scratch, float* centers_new, float* cnorm, int* counts, double* inertia,
                         hipStream_t stream) {
    const KmPlan p = km_plan(N, K, D);
    char* base = (char*)scratch;
    int* hist = (int*)(base + p.off_hist);
    int* ccount = (int*)(base + p.off_ccount);
    int* cstart = (int*)(base + p.off_cstart);
    int* pstart = (int*)(base + p.off_pstart);
    int* perm = (int*)(base + p.off_perm);
    double* ipart = (double*)(base + p.off_ipart);
    double* part = (double*)(base + p.off_part);
    km_hist_kernel<<<p.NB, 256, 0, stream>>>(labels, dist, N, K, p.RB, hist, ipart);
    CPC_CHECK_LAUNCH();
    km_blockscan_kernel<<<K, 64, 0, stream>>>(hist, p.NB, K, ccount);
    CPC_CHECK_LAUNCH();
    km_offsets_kernel<<<1, 1024, 0, stream>>>(ccount, K, p.PL, cstart, pstart, ipart, p.NB, inertia);
    CPC_CHECK_LAUNCH();
    km_rank_kernel<<<p.NB, 64, 0, stream>>>(labels, N, K, p.RB, hist, cstart, perm);
    CPC_CHECK_LAUNCH();
    if (dtype == CPC_DTYPE_BF16)
        km_segsum_kernel<bf16_t><<<(unsigned)p.PMAX, 256, 0, stream>>>((const bf16_t*)x, D, ldx, K, p.PL, perm, cstart, pstart, part);
    else
        km_segsum_kernel<float><<<(unsigned)p.PMAX, 256, 0, stream>>>((const float*)x, D, ldx, K, p.PL, perm, cstart, pstart, part);
    CPC_CHECK_LAUNCH();
    km_fold_kernel<<<K, 256, 0, stream>>>(part, cstart, pstart, centers_old, D, centers_new, cnorm, counts);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

int launch_kmeans_cnorm(const float* centers, float* cnorm, int K, int D, hipStream_t stream) {
    km_cnorm_kernel<<<K, 256, 0, stream>>>(centers, D, cnorm);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
