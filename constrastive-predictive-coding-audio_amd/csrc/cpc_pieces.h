// Pieces of four consecutive samples, as the sample gathers move them (dataset.hip: cpc_window_gather; stream.hip: cpc_stream_gather):
// read from an address that is aligned to one sample only, converted to f32, stored as 16 bytes where the output row allows.
#pragma once
#include "cpc_common.h"

constexpr int WG_PIECE = 4;                           // outputs per piece: one 16-byte store

// Four consecutive samples from an address aligned to one sample only.
template <typename T> struct WgPiece { T v[WG_PIECE]; };
template <typename T>
__device__ __forceinline__ WgPiece<T> wg_load(const T* src) {
    WgPiece<T> p;
    __builtin_memcpy(&p, src, sizeof(p));
    return p;
}

// COPY: the f32 store with scale 1, moved bit for bit (a multiplication by 1 would quiet a signalling NaN).
template <typename T, bool COPY>
__device__ __forceinline__ float wg_value(T s, float scale) {
    return COPY ? (float)s : (float)s * scale;
}
