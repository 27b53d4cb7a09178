// gs_sort_key.h -- the layouts of a sort key in the K-domain arrays (keys_a / keys_b), stated once for host and device.
//
// The WIDE key of a pair is (tile << depth_bits) | depth_code in a uint32_t, or a uint64_t when depth_bits + tile bits > 32
// (k_binning.hip); its order is that of the reference's (tile << 32) + depth_code (RAST:169-170), which the export rebuilds.
//
// The NARROW key is the wide key without its low byte, in a uint16_t:
//     narrow = wide >> 8 = (tile << (depth_bits - 8)) | (depth_code >> 8)
// It exists where k_keygen has already placed every pair by digit 0, the low byte of the depth code (first pass, depth_bits >= 8):
// from there on the sort looks at (wide >> shift) & 255 with shift >= 8 only, which is (narrow >> (shift - 8)) & 255, and the
// tile search at wide >> depth_bits, which is narrow >> (depth_bits - 8).  The low byte is not lost: it is the low byte of the
// pair's point's depth code, which the frame keeps per point (depth_codes[vals_sorted[i]]).
// A frame takes the narrow class when the first pass is k_keygen's and the remaining key_bits - 8 bits fit 16.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_KEY_FN __host__ __device__ __forceinline__
#else
#define GS_KEY_FN static inline
#endif

#define GS_NARROW_DROPPED_BITS 8        // digit 0: placed by k_keygen, never read again
#define GS_NARROW_KEY_BITS 16

// bytes of one element of keys_a / keys_b: 2 (narrow), 4 or 8.  key_bits = depth_bits + tile bits; first_pass: k_keygen does the
// pass over digit 0 (a digit table exists for this frame); narrow_allowed: the GS_SORT_NARROW_KEYS switch.
GS_KEY_FN int gs_key_bytes(int key_bits, int depth_bits, bool first_pass, bool narrow_allowed)
{
    if (narrow_allowed && first_pass && depth_bits >= GS_NARROW_DROPPED_BITS && key_bits - GS_NARROW_DROPPED_BITS <= GS_NARROW_KEY_BITS) return 2;
    return key_bits > 32 ? 8 : 4;
}

// what the sort shifts and the tile search see of a key of `key_bytes` bytes: bit b of the wide key is bit b - gs_key_dropped_bits of the stored one
GS_KEY_FN int gs_key_dropped_bits(int key_bytes) { return key_bytes == 2 ? GS_NARROW_DROPPED_BITS : 0; }

GS_KEY_FN uint64_t gs_wide_key(uint32_t tile, uint32_t code, int depth_bits) { return ((uint64_t)tile << depth_bits) | (uint64_t)code; }

// (a depth code wider than depth_bits, or a tile beyond the 16 bits, belongs to a frame whose sizes were predicted too small and is
// rendered again: the value is truncated, as the wide store truncates to its word)
GS_KEY_FN uint16_t gs_narrow_key(uint32_t tile, uint32_t code, int depth_bits)
{
    return (uint16_t)((tile << (depth_bits - GS_NARROW_DROPPED_BITS)) | (code >> GS_NARROW_DROPPED_BITS));
}

GS_KEY_FN uint32_t gs_narrow_tile(uint16_t narrow, int depth_bits) { return (uint32_t)narrow >> (depth_bits - GS_NARROW_DROPPED_BITS); }

// the wide key again, from the narrow one and the depth code of the pair's point
GS_KEY_FN uint32_t gs_wide_of_narrow(uint16_t narrow, uint32_t code) { return ((uint32_t)narrow << GS_NARROW_DROPPED_BITS) | (code & 255u); }

// the reference's 64-bit key, RAST:169-170
GS_KEY_FN int64_t gs_reference_key(uint32_t tile, uint32_t code) { return (int64_t)code + ((int64_t)tile << 32); }
