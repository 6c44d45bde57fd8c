// Fused four-gate LSTM recurrence (AudioLSTMModel's context network), forward and backward through time.
//
// torch.nn.LSTMCell, gate order i, f, g, o.  With a = Gi[:, t] + h_{t-1} W_hh^T + b_hh:
//   i = sigmoid(a_i), f = sigmoid(a_f), g = tanh(a_g), o = sigmoid(a_o), cell_t = f cell_{t-1} + i g, h_t = o tanh(cell_t).
// The input projection x_t W_ih^T + b_ih is one batched gemm_nt over all V steps (done by the caller).  The recurrence runs here in
// the form of the weight-streaming GRU kernels (gru.hip): ONE persistent launch per direction, a workgroup owns 16 batch rows for
// all V steps, keeps h and cell (f32 masters in registers; a storage-dtype copy of h in LDS, double-buffered, as the MFMA operand)
// on chip and streams W_hh, pre-arranged in MFMA fragment order by cpc_prep_frag, from L2.
//
// MFMA orientation: D[row = gate column][col = batch row]; a lane holds the four pre-activations of the same (batch row, hidden
// unit) quadruple in four accumulators and does the gate math without any exchange.
#include "cpc_common.h"
#include "cpc_kernels.h"

namespace {

constexpr int LSTM_MAXJT = 4;      // hidden tiles (16 units) per wave -> H <= 256 with 4 waves, H <= 512 with 8
constexpr int LSTM_SLOTS = 6;      // tape [b][t][i, f, g, o, cell_{t-1}, tanh(cell_t)][H]

template <typename T>
__device__ __forceinline__ uint4 ldg16(const T* p) { return *(const uint4*)p; }

// LDS of one workgroup, sized for the largest H of its family (HMAX = 256 with NW = 4, 512 with NW = 8): static, so that no launch
// asks for more dynamic LDS than the default limit grants (the backward tile is 65 792 B at (f32, 256) and (bf16, 512)).
template <typename T, int HMAX> struct LstmLds {
    static constexpr int FWD = 2 * 16 * (HMAX * (int)sizeof(T) + 16) + 4 * HMAX * (int)sizeof(float);
    static constexpr int BWD = 16 * (4 * HMAX * (int)sizeof(T) + 16);
};

// NW waves per workgroup: wave w owns the hidden tiles w + NW*q, q < LSTM_MAXJT.  grid: ceil(B/16); block 64 * NW.
template <typename T, int NW>
__device__ __forceinline__ void lstm_fwd_steps(unsigned char* smem, const T* __restrict__ Gi, const T* __restrict__ Wfrag,
                                               const float* __restrict__ bhh, const float* __restrict__ h0,
                                               const float* __restrict__ c0, T* __restrict__ Hall, T* __restrict__ tape,
                                               float* __restrict__ h_out, float* __restrict__ cell_out, int B, int V, int H) {
    constexpr int CH = Elem<T>::CH, NTHR = 64 * NW;
    const int rowb = H * (int)sizeof(T) + 16;             // h tile row stride in bytes (16 B pad)
    unsigned char* hbuf[2] = {smem, smem + 16 * rowb};
    float* bsh = (float*)(smem + 2 * 16 * rowb);           // b_hh [4H]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fg = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const int b = b0 + frow;
    const bool b_ok = b < B;
    const int ntile = H / 16;
    const int KC = H / (4 * CH);

    for (int i = tid; i < 4 * H; i += NTHR) bsh[i] = bhh ? bhh[i] : 0.f;
    // h_0 (the carried state, or zeros) into the first tile and into Hall[:, 0, :]; the second tile is written by step 0
    for (int i = tid; i < 16 * H; i += NTHR) {
        const int rb = i / H, j = i % H;
        const float v = (h0 && b0 + rb < B) ? h0[(long long)(b0 + rb) * H + j] : 0.f;
        ((T*)(hbuf[0] + rb * rowb))[j] = from_f32<T>(v);
        if (b0 + rb < B) Hall[((long long)(b0 + rb) * (V + 1)) * H + j] = from_f32<T>(v);
    }
    __syncthreads();

    // the f32 master of cell lives in registers for the whole sequence (that of h is consumed within its step: h enters the next
    // step only through the MFMA operand, the rounded copy in LDS)
    float cell[LSTM_MAXJT][4];
#pragma unroll
    for (int q = 0; q < LSTM_MAXJT; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int jt = wave + NW * q;
            cell[q][e] = (c0 && b_ok && jt < ntile) ? c0[(long long)b * H + jt * 16 + fg * 4 + e] : 0.f;
        }

    for (int t = 0; t < V; ++t) {
        const unsigned char* hcur = hbuf[t & 1];
        unsigned char* hnext = hbuf[(t + 1) & 1];
        const T* girow = Gi + ((long long)b * V + t) * 4 * H + fg * 4;
        // input-projection terms of this step (issued early; consumed after the MFMA loop)
        f32x4 gi[LSTM_MAXJT][4];
#pragma unroll
        for (int q = 0; q < LSTM_MAXJT; ++q) {
            const int jt = wave + NW * q;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                gi[q][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (jt < ntile && b_ok) gi[q][g] = load4(girow + g * H + jt * 16);
            }
        }
        f32x4 acc[LSTM_MAXJT][4];
#pragma unroll
        for (int q = 0; q < LSTM_MAXJT; ++q) {
            const int jt = wave + NW * q;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                acc[q][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (jt < ntile) acc[q][g] = *(const f32x4*)(bsh + g * H + jt * 16 + fg * 4);
            }
        }

        for (int kc = 0; kc < KC; ++kc) {
            const uint4 hf = *(const uint4*)(hcur + frow * rowb + (kc * 4 + fg) * 16);
#pragma unroll
            for (int q = 0; q < LSTM_MAXJT; ++q) {
                const int jt = wave + NW * q;
                if (jt < ntile) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int nt = g * ntile + jt;
                        const uint4 wf = ldg16(Wfrag + ((long long)(nt * KC + kc) * 64 + lane) * CH);
                        mfma_chunk<T>(acc[q][g], wf, hf);
                    }
                }
            }
        }
        // gate math for (b, j = jt*16 + fg*4 + e)
#pragma unroll
        for (int q = 0; q < LSTM_MAXJT; ++q) {
            const int jt = wave + NW * q;
            if (jt < ntile) {
                const int j = jt * 16 + fg * 4;
                const f32x4* gq = gi[q];
                f32x4 i4, f4, g4, o4, cp4, tc4, h4, c4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ig = fast_sigmoid(gq[0][e] + acc[q][0][e]);
                    const float fo = fast_sigmoid(gq[1][e] + acc[q][1][e]);
                    const float gg = fast_tanh(gq[2][e] + acc[q][2][e]);
                    const float og = fast_sigmoid(gq[3][e] + acc[q][3][e]);
                    const float cp = cell[q][e];
                    const float cn = fo * cp + ig * gg;
                    const float tc = fast_tanh(cn);
                    const float hn = og * tc;
                    cell[q][e] = cn;
                    i4[e] = ig; f4[e] = fo; g4[e] = gg; o4[e] = og; cp4[e] = cp; tc4[e] = tc; h4[e] = hn; c4[e] = cn;
                }
                store4((T*)(hnext + frow * rowb) + j, h4);
                if (b_ok) {
                    store4(Hall + ((long long)b * (V + 1) + (t + 1)) * H + j, h4);
                    T* gp = tape + (((long long)b * V + t) * LSTM_SLOTS) * H + j;
                    store4(gp, i4);
                    store4(gp + H, f4);
                    store4(gp + 2 * H, g4);
                    store4(gp + 3 * H, o4);
                    store4(gp + 4 * H, cp4);
                    store4(gp + 5 * H, tc4);
                    if (t == V - 1) {
                        *(f32x4*)(h_out + (long long)b * H + j) = h4;
                        *(f32x4*)(cell_out + (long long)b * H + j) = c4;
                    }
                }
            }
        }
        __syncthreads();
    }
}

template <typename T, int NW>
__global__ __launch_bounds__(64 * NW) void lstm_fwd_kernel(const T* __restrict__ Gi, const T* __restrict__ Wfrag,
                                                           const float* __restrict__ bhh, const float* __restrict__ h0,
                                                           const float* __restrict__ c0, T* __restrict__ Hall,
                                                           T* __restrict__ tape, float* __restrict__ h_out,
                                                           float* __restrict__ cell_out, int B, int V, int H) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[LstmLds<T, 64 * NW>::FWD];
    lstm_fwd_steps<T, NW>(smem, Gi, Wfrag, bhh, h0, c0, Hall, tape, h_out, cell_out, B, V, H);
}

// WTfrag: fragment-ordered W_hh^T ([H][4H] logical: rows = hidden unit, k = gate column).
// STEPS (cpc_lstm_bwd_steps: predictions from several context steps): a gradient arrives at every hidden state,
// dHs[(b V + t) ld_h + j] at h_{t+1}, and joins dh at the top of step t; dh_last may then be NULL (zeros).  STEPS == false is
// cpc_lstm_bwd's code: dHs / ld_h are not read.
template <typename T, int NW, bool STEPS>
__device__ __forceinline__ void lstm_bwd_steps(unsigned char* smem, const float* __restrict__ dh_last, const T* __restrict__ tape,
                                               const T* __restrict__ WTfrag, T* __restrict__ dG, int B, int V, int H,
                                               const T* __restrict__ dHs, long long ld_h) {
    constexpr int CH = Elem<T>::CH;
    const int rowb = 4 * H * (int)sizeof(T) + 16;
    unsigned char* gcur = smem;                            // gate-gradient tile [16][4H] (+16 B pad per row)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fg = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const int b = b0 + frow;
    const bool b_ok = b < B;
    const int ntile = H / 16;
    const int KC = 4 * H / (4 * CH);

    float dh[LSTM_MAXJT][4], dcell[LSTM_MAXJT][4];
#pragma unroll
    for (int q = 0; q < LSTM_MAXJT; ++q) {
        const int jt = wave + NW * q;
#pragma unroll
        for (int e = 0; e < 4; ++e) { dh[q][e] = 0.f; dcell[q][e] = 0.f; }
        if (jt < ntile && b_ok && (!STEPS || dh_last)) {
            const f32x4 v = *(const f32x4*)(dh_last + (long long)b * H + jt * 16 + fg * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) dh[q][e] = v[e];
        }
    }

    for (int t = V - 1; t >= 0; --t) {
#pragma unroll
        for (int q = 0; q < LSTM_MAXJT; ++q) {
            const int jt = wave + NW * q;
            if (jt < ntile) {
                const int j = jt * 16 + fg * 4;
                f32x4 i4 = (f32x4){0.f, 0.f, 0.f, 0.f}, f4 = i4, g4 = i4, o4 = i4, cp4 = i4, tc4 = i4;
                if (b_ok) {          // rows of items >= B are not read (as the stores of dG are masked)
                    const T* gp = tape + (((long long)b * V + t) * LSTM_SLOTS) * H + j;
                    i4 = load4(gp); f4 = load4(gp + H); g4 = load4(gp + 2 * H); o4 = load4(gp + 3 * H);
                    cp4 = load4(gp + 4 * H); tc4 = load4(gp + 5 * H);
                    if constexpr (STEPS) {          // rows of items >= B and columns [H, ld_h) are not read
                        const f32x4 ds = load4(dHs + ((long long)b * V + t) * ld_h + j);
#pragma unroll
                        for (int e = 0; e < 4; ++e) dh[q][e] += ds[e];
                    }
                }
                f32x4 di4, df4, dg4, do4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = dh[q][e];
                    const float ig = i4[e], fo = f4[e], gg = g4[e], og = o4[e], tc = tc4[e];
                    const float do_pre = d * tc * og * (1.f - og);
                    const float dct = dcell[q][e] + d * og * (1.f - tc * tc);
                    di4[e] = dct * gg * ig * (1.f - ig);
                    df4[e] = dct * cp4[e] * fo * (1.f - fo);
                    dg4[e] = dct * ig * (1.f - gg * gg);
                    do4[e] = do_pre;
                    dcell[q][e] = dct * fo;
                }
                T* grow = (T*)(gcur + frow * rowb);
                store4(grow + j, di4);
                store4(grow + H + j, df4);
                store4(grow + 2 * H + j, dg4);
                store4(grow + 3 * H + j, do4);
                if (b_ok) {
                    T* go = dG + ((long long)b * V + t) * 4 * H + j;          // [di | df | dg | do]
                    store4(go, di4); store4(go + H, df4); store4(go + 2 * H, dg4); store4(go + 3 * H, do4);
                }
            }
        }
        __syncthreads();
        // dh_{t-1} = [di | df | dg | do]_pre * W_hh
        f32x4 acc[LSTM_MAXJT];
#pragma unroll
        for (int q = 0; q < LSTM_MAXJT; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};

        for (int kc = 0; kc < KC; ++kc) {
            const uint4 gf = *(const uint4*)(gcur + frow * rowb + (kc * 4 + fg) * 16);
#pragma unroll
            for (int q = 0; q < LSTM_MAXJT; ++q) {
                const int jt = wave + NW * q;
                if (jt < ntile) {
                    const uint4 wf = ldg16(WTfrag + ((long long)(jt * KC + kc) * 64 + lane) * CH);
                    mfma_chunk<T>(acc[q], wf, gf);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < LSTM_MAXJT; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) dh[q][e] = acc[q][e];
        __syncthreads();      // all reads of the tile are done before the next step overwrites it
    }
}

template <typename T, int NW, bool STEPS>
__global__ __launch_bounds__(64 * NW) void lstm_bwd_kernel(const float* __restrict__ dh_last, const T* __restrict__ tape,
                                                           const T* __restrict__ WTfrag, T* __restrict__ dG, int B, int V, int H,
                                                           const T* __restrict__ dHs, long long ld_h) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[LstmLds<T, 64 * NW>::BWD];
    lstm_bwd_steps<T, NW, STEPS>(smem, dh_last, tape, WTfrag, dG, B, V, H, dHs, ld_h);
}

constexpr int LSTM_LDS_LIMIT = 160 * 1024;          // LDS of one gfx950 CU
static_assert(LstmLds<float, 512>::BWD <= LSTM_LDS_LIMIT && LstmLds<float, 512>::FWD <= LSTM_LDS_LIMIT, "the widest tiles fit one CU");

}  // namespace

static bool lstm_ok(int B, int V, int H, int dtype) {
    if (dtype != CPC_DTYPE_BF16 && dtype != CPC_DTYPE_F32) return false;
    const int ch = dtype == CPC_DTYPE_BF16 ? 8 : 4;
    if (B <= 0 || V <= 0 || H <= 0) return false;
    return H % 16 == 0 && H % (4 * ch) == 0 && H <= 64 * 8;
}

long long lstm_tape_elems(int B, int V, int H, int dtype) {
    if (!lstm_ok(B, V, H, dtype)) return CPC_EINVAL;
    return (long long)B * V * LSTM_SLOTS * H;
}

int launch_lstm_fwd(const void* Gi, const void* Wfrag, const float* bhh, const float* h0, const float* c0, void* Hall, void* tape,
                    float* h_out, float* cell_out, int B, int V, int H, int dtype, hipStream_t stream) {
    if (!lstm_ok(B, V, H, dtype)) return CPC_EINVAL;
    const dim3 grid((B + 15) / 16);
#define LSTM_F(T, NW) \
    hipLaunchKernelGGL((lstm_fwd_kernel<T, NW>), grid, dim3(64 * NW), 0, stream, (const T*)Gi, (const T*)Wfrag, bhh, h0, c0, \
                       (T*)Hall, (T*)tape, h_out, cell_out, B, V, H)
    if (H > 256) {          // 8 waves (tiles w + 8q): two waves per SIMD
        if (dtype == CPC_DTYPE_BF16) LSTM_F(bf16_t, 8); else LSTM_F(float, 8);
    } else {
        if (dtype == CPC_DTYPE_BF16) LSTM_F(bf16_t, 4); else LSTM_F(float, 4);
    }
#undef LSTM_F
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}

// dHs == NULL: cpc_lstm_bwd's kernels.  Otherwise the STEPS instantiations of the same body, chosen the same way.
int launch_lstm_bwd(const float* dh_last, const void* tape, const void* WTfrag, void* dG, int B, int V, int H, int dtype,
                    hipStream_t stream, const void* dHs, long long ld_h) {
    if (!lstm_ok(B, V, H, dtype)) return CPC_EINVAL;
    if (!dHs && !dh_last) return CPC_EINVAL;
    if (dHs && (ld_h < H || ld_h % (dtype == CPC_DTYPE_BF16 ? 8 : 4))) return CPC_EINVAL;
    const dim3 grid((B + 15) / 16);
#define LSTM_B(T, NW, STEPS) \
    hipLaunchKernelGGL((lstm_bwd_kernel<T, NW, STEPS>), grid, dim3(64 * NW), 0, stream, dh_last, (const T*)tape, (const T*)WTfrag, \
                       (T*)dG, B, V, H, (const T*)dHs, ld_h)
#define LSTM_BS(T, NW) do { if (dHs) LSTM_B(T, NW, true); else LSTM_B(T, NW, false); } while (0)
    if (H > 256) {
        if (dtype == CPC_DTYPE_BF16) LSTM_BS(bf16_t, 8); else LSTM_BS(float, 8);
    } else {
        if (dtype == CPC_DTYPE_BF16) LSTM_BS(bf16_t, 4); else LSTM_BS(float, 4);
    }
#undef LSTM_BS
#undef LSTM_B
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
