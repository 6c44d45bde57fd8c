// Counter-based draws shared by the waveform augmentation (augment.hip) and the grid masking (gridmask.hip): every random number is
// a pure function of (seed, step, clip, field), with the arithmetic of drop_hash (attn.hip) and of the sampled negatives (nce.hip);
// include/cpc_hip.h states it with cpc_wave_augment.
#pragma once
#include "cpc_common.h"

namespace {

typedef unsigned long long u64;

constexpr u64 WA_DRAW = 0x632BE59BD9B4E019ull, WA_STEP = 0x9E3779B97F4A7C15ull, WA_IDX = 0xD1B54A32D192ED03ull;

__host__ __device__ __forceinline__ u64 wa_mix(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// kb of clip clip_offset + b
__device__ __forceinline__ u64 wa_key(u64 seed, u64 step, u64 clip_offset, int b) {
    return wa_mix(seed + WA_DRAW * step + WA_STEP * (clip_offset + (u64)b + 1ull));
}
__device__ __forceinline__ unsigned wa_field(u64 kb, u64 f) { return (unsigned)(wa_mix(kb + WA_IDX * f) >> 32); }
__device__ __forceinline__ int wa_int(unsigned u, int lo, int hi) { return lo + (int)(((u64)u * (u64)(hi - lo + 1)) >> 32); }
__device__ __forceinline__ float wa_real(unsigned u, float lo, float hi) { return fmaf(hi - lo, (float)u * 0x1p-32f, lo); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
