// Device-resident audio dataset (include/cpc_hip.h, cpc_window_gather; DESIGN.md, "Device-resident audio dataset"): a batch of
// overlapping windows cut out of the concatenated samples of every file, converted to f32 on the way.  Memory-bound by design: every
// output is written once and its sample read once.  Grid row b is output row b, so the two table reads of a row (its example index,
// the example's first sample) are the same in every lane of a workgroup; a lane moves pieces of four consecutive samples.  A window
// starts at an arbitrary sample: the source of a piece is only aligned to one sample (2 bytes for int16, 4 for f32), so a piece is
// read with a copy of unknown alignment that the compiler lowers to what the target allows, and stored as 16 bytes where the output
// row allows.  No LDS, no atomics.
#include <cmath>
#include "cpc_common.h"
#include "cpc_draws.h"
#include "cpc_kernels.h"
#include "cpc_pieces.h"
#include "../../include/cpc_hip.h"

namespace {

// Workgroup (blockIdx.x, blockIdx.y): outputs [tile blockIdx.x, +tile) of row blockIdx.y, tile = 4 ITERS blockDim.x; a lane ITERS pieces
// of 4, blockDim.x pieces apart.  The row reads the store only where its whole window [s, s + L) lies inside it, and is zeros otherwise.
template <typename T, bool COPY, int ITERS>
__global__ __launch_bounds__(256) void window_gather_kernel(const T* __restrict__ store, long long store_len,
                                                            const long long* __restrict__ starts, long long n_items,
                                                            const long long* __restrict__ idx, float* __restrict__ out, int L,
                                                            long long ldo, float scale, int vec_out) {
    const int b = blockIdx.y;
    const long long i = idx[b];
    long long s = -1;
    if (i >= 0 && i < n_items) s = starts[i];
    const bool inside = s >= 0 && s <= store_len - L;          // store_len >= L (checked by the entry point)
    const T* src = store + (inside ? s : 0);
    float* row = out + (long long)b * ldo;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int n0 = WG_PIECE * (((int)blockIdx.x * ITERS + it) * (int)blockDim.x + (int)threadIdx.x);
        if (n0 >= L) continue;
        const bool whole = n0 + WG_PIECE - 1 < L;
        float v[WG_PIECE] = {0.f, 0.f, 0.f, 0.f};
        if (inside) {
            if (whole) {
                const WgPiece<T> p = wg_load(src + n0);
#pragma unroll
                for (int j = 0; j < WG_PIECE; ++j) v[j] = wg_value<T, COPY>(p.v[j], scale);
            } else {
#pragma unroll
                for (int j = 0; j < WG_PIECE; ++j)
                    if (n0 + j < L) v[j] = wg_value<T, COPY>(src[n0 + j], scale);
            }
        }
        if (vec_out && whole) {
            *(f32x4*)(row + n0) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int j = 0; j < WG_PIECE; ++j)
                if (n0 + j < L) row[n0 + j] = v[j];
        }
    }
}

template <typename T, bool COPY>
void window_gather_launch(const void* store, long long store_len, const long long* starts, long long n_items, const long long* idx,
                          float* out, int B, int L, long long ldo, float scale, hipStream_t stream) {
    const int vec_out = aligned16(out) && ldo % 4 == 0;
    const T* st = (const T*)store;
    // The grid follows B L, not B: tiles of 4096 outputs (four pieces in flight per lane) where that still gives every CU several
    // workgroups, tiles of 1024 below that, and single waves (256 outputs) for the smallest batches.
    const long long want = 1024;
    auto tiles = [&](int tile) { return (long long)B * ((L + tile - 1) / tile); };
    if (tiles(4096) >= want) {
        window_gather_kernel<T, COPY, 4><<<dim3((L + 4095) / 4096, B), 256, 0, stream>>>(st, store_len, starts, n_items, idx, out, L, ldo,
                                                                                          scale, vec_out);
    } else if (tiles(1024) >= want) {
        window_gather_kernel<T, COPY, 1><<<dim3((L + 1023) / 1024, B), 256, 0, stream>>>(st, store_len, starts, n_items, idx, out, L, ldo,
                                                                                          scale, vec_out);
    } else {
        window_gather_kernel<T, COPY, 1><<<dim3((L + 255) / 256, B), 64, 0, stream>>>(st, store_len, starts, n_items, idx, out, L, ldo,
                                                                                       scale, vec_out);
    }
}

}  // namespace

int launch_window_gather(const void* store, int store_code, long long store_len, const long long* starts, long long n_items,
                         const long long* idx, float* out, int B, int L, long long ldo, float scale, hipStream_t stream) {
    if (store_code == 1)
        window_gather_launch<short, false>(store, store_len, starts, n_items, idx, out, B, L, ldo, scale, stream);
    else if (scale == 1.0f)
        window_gather_launch<float, true>(store, store_len, starts, n_items, idx, out, B, L, ldo, scale, stream);
    else
        window_gather_launch<float, false>(store, store_len, starts, n_items, idx, out, B, L, ldo, scale, stream);
    CPC_CHECK_LAUNCH();
    return CPC_OK;
}
