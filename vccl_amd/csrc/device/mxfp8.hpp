// MXFP8 wire codec: 32-element blocks of OCP E4M3 under one
// E8M0 scale byte, laid out in tiles of 512 elements = 512 payload bytes
// followed by one 16-byte line of the tile's 16 scale bytes (528 bytes, 33
// lines of 16).  Payload byte i of a tile is element i, scale byte j its block
// j.  Blocks are cut by GLOBAL element index; a short last block counts its
// missing elements as 0.
//
//   block of finite values, amax = max |v| (binary32):
//     amax == 0: s = 127, payload 0; else e = the smallest integer with
//     amax * 2^-e <= 448 — exponent field F of amax: e + 127 = F - 8, plus 1
//     when the fraction field exceeds 0x600000 (1.75 = 448 / 256) —
//     s = max(e + 127, 0) (the top clamp 254 is never reached: F <= 254 gives
//     at most 247), payload byte i = E4M3(v_i * 2^(127 - s)), RN-even;
//   a block holding a NaN or an infinity: s = 255, payload 0, every element
//     decodes to NaN;
//   decode: widen(byte) * 2^(s - 127), exact in binary32.
// Nothing saturates: amax * 2^(127 - s) <= 448 by construction (s = 0 is only
// reached below 2^-119, where the product stays below 2^8).  Values below
// 2^-100 may flush to zero (binary32 subnormal products).
//
// The scaled narrowing is v_mul_f32 by the exact power of two and
// v_cvt_pk_fp8_f32 (the converter ops.hpp's E4M3 sums already use: RN-even, no
// input above 448 ever reaches it here), the widening v_cvt_pk_f32_fp8 and a
// multiply: both products are exact, so the bits are the contract's.
//
// Lane mapping: one wave handles one tile per step, lane l the 8 elements
// [8 l, 8 l + 8) = 8 payload bytes; a block is one quad of lanes, its amax two
// DPP quad_perm steps on the magnitude bits (integer compare: NaN and infinity
// order above every finite value).  The tile's 16 scale bytes are read out of
// lanes 0, 4, ..., 60 with v_readlane into one 16-byte store by lane 0.  Every
// function here is called by ALL 64 lanes of a wave (wave-uniform control flow).
#pragma once
#include "coll_types.hpp"
#include "reduce_copy.hpp"

namespace vccl {

// One element up to / down from binary32 (down: the native RN-even narrowing).
template <typename T> struct MxElt {
  static __device__ __forceinline__ float up(T x) { return Wide<T>::up(x); }
  static __device__ __forceinline__ T down(float f) { return Wide<T>::down(f); }
};
template <> struct MxElt<float> {
  static __device__ __forceinline__ float up(float x) { return x; }
  static __device__ __forceinline__ float down(float f) { return f; }
};

// This lane's 8 elements, p = the address of the first, nValid of them exist (<= 0: none; the others read as 0).
// vec: p is 16-byte aligned (wave-uniform: a tile starts on a multiple of 16 bytes from the buffer's base).
template <typename T, int LDP>
__device__ __forceinline__ void mx_load8(const char* p, int64_t nValid, bool vec, float (&v)[8]) {
  if (vec && nValid >= 8) {
    if constexpr (sizeof(T) == 4) {
      const u32x4 a = ld16<LDP>(p, 0), b = ld16<LDP>(p, 16);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t wa = a[k], wb = b[k];  // a copy first: bit_cast of the vector element itself read element 0
        v[k] = __builtin_bit_cast(float, wa);
        v[4 + k] = __builtin_bit_cast(float, wb);
      }
    } else {
      const u32x4 a = ld16<LDP>(p, 0);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        f32x2 q;
        Wide<T>::up_word(a[k], &q);
        v[2 * k] = q.x;
        v[2 * k + 1] = q.y;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = j < nValid ? MxElt<T>::up(ldT<LDP, T>(p, j)) : 0.0f;
  }
}
// ... narrowed and stored; only the nValid existing elements are written.
template <typename T, int STP>
__device__ __forceinline__ void mx_store8(char* p, int64_t nValid, bool vec, const float (&v)[8]) {
  if (vec && nValid >= 8) {
    if constexpr (sizeof(T) == 4) {
      u32x4 a, b;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float fa = v[k], fb = v[4 + k];
        a[k] = __builtin_bit_cast(uint32_t, fa);
        b[k] = __builtin_bit_cast(uint32_t, fb);
      }
      st16<STP>(p, 0, a);
      st16<STP>(p, 16, b);
    } else {
      u32x4 a;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const f32x2 q{v[2 * k], v[2 * k + 1]};
        a[k] = Wide<T>::down_word(&q);
      }
      st16<STP>(p, 0, a);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (j < nValid) stT<STP, T>(p, j, MxElt<T>::down(v[j]));
  }
}

__device__ __forceinline__ uint32_t mx_quad_max(uint32_t a) {
  uint32_t b = (uint32_t)__builtin_amdgcn_mov_dpp((int)a, 0xB1, 0xf, 0xf, true);  // quad_perm [1, 0, 3, 2]
  a = a > b ? a : b;
  b = (uint32_t)__builtin_amdgcn_mov_dpp((int)a, 0x4E, 0xf, 0xf, true);  // quad_perm [2, 3, 0, 1]
  return a > b ? a : b;
}

// Encode this lane's 8 values of its quad's block: payload words lo (elements 0 .. 3) / hi, scale byte s.
__device__ __forceinline__ void mx_encode8(const float (&v)[8], uint32_t& lo, uint32_t& hi, uint32_t& s) {
  uint32_t amax = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint32_t m = __builtin_bit_cast(uint32_t, v[j]) & 0x7fffffffu;
    amax = amax > m ? amax : m;
  }
  amax = mx_quad_max(amax);
  if (amax >= 0x7f800000u) {  // a NaN or an infinity in the block
    s = 255;
    lo = hi = 0;
    return;
  }
  int e = (int)(amax >> 23) - 8 + ((amax & 0x7fffffu) > 0x600000u ? 1 : 0);
  s = amax == 0 ? 127u : (uint32_t)(e < 0 ? 0 : e);
  const float mul = __builtin_bit_cast(float, (254u - s) << 23);  // 2^(127 - s), s <= 247
  int r = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * mul, v[1] * mul, 0, false);
  lo = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[2] * mul, v[3] * mul, r, true);
  r = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * mul, v[5] * mul, 0, false);
  hi = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[6] * mul, v[7] * mul, r, true);
}
__device__ __forceinline__ void mx_decode8(uint32_t lo, uint32_t hi, uint32_t s, float (&v)[8]) {
  // 2^(s - 127): s = 0 is the binary32 subnormal 2^-127, s = 255 a NaN (0 * NaN = NaN: the whole block)
  const float mul = __builtin_bit_cast(float, s == 255 ? 0x7fc00000u : s == 0 ? 0x00400000u : s << 23);
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  v[0] = a.x * mul;
  v[1] = a.y * mul;
  v[2] = b.x * mul;
  v[3] = b.y * mul;
  v[4] = c.x * mul;
  v[5] = c.y * mul;
  v[6] = d.x * mul;
  v[7] = d.y * mul;
}

// The wire tile at `tile` (16-byte aligned): this lane's 8 payload bytes, and the scale line by lane 0.
template <int STP>
__device__ __forceinline__ void mx_store_tile(char* tile, int lane, uint32_t lo, uint32_t hi, uint32_t s) {
  stT<STP, uint64_t>(tile, lane, (uint64_t)hi << 32 | lo);
  u32x4 line = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 16; j++) line[j / 4] |= (uint32_t)__builtin_amdgcn_readlane((int)s, 4 * j) << (8 * (j % 4));
  if (lane == 0) st16<STP>(tile, kMxTileElts, line);
}
template <int LDP>
__device__ __forceinline__ void mx_load_tile(const char* tile, int lane, uint32_t& lo, uint32_t& hi, uint32_t& s) {
  const uint64_t x = ldT<LDP, uint64_t>(tile, lane);
  lo = (uint32_t)x;
  hi = (uint32_t)(x >> 32);
  s = ldT<LDP, uint8_t>(tile + kMxTileElts, lane >> 2);
}

// The codec on its own (vcclMxfp8Pack / vcclMxfp8Unpack): one wave per tile, grid-stride; the user buffer at any
// element alignment (off 16 bytes: the element path), the wire 16-byte aligned, written / read in whole tiles.
template <typename T>
__device__ __forceinline__ void mxfp8_pack(const char* src, char* wire, int64_t count) {
  const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int64_t gw = (int64_t)blockIdx.x * nw + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nTiles = (count + kMxTileElts - 1) / kMxTileElts;
  const bool vec = ((uintptr_t)src & 15) == 0;
  for (int64_t t = gw; t < nTiles; t += (int64_t)gridDim.x * nw) {
    const int64_t i0 = t * kMxTileElts + lane * 8;
    float v[8];
    mx_load8<T, kPlain>(src + i0 * (int64_t)sizeof(T), count - i0, vec, v);
    uint32_t lo, hi, s;
    mx_encode8(v, lo, hi, s);
    mx_store_tile<kPlain>(wire + t * kMxTileBytes, lane, lo, hi, s);
  }
}
template <typename T>
__device__ __forceinline__ void mxfp8_unpack(const char* wire, char* dst, int64_t count) {
  const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int64_t gw = (int64_t)blockIdx.x * nw + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nTiles = (count + kMxTileElts - 1) / kMxTileElts;
  const bool vec = ((uintptr_t)dst & 15) == 0;
  for (int64_t t = gw; t < nTiles; t += (int64_t)gridDim.x * nw) {
    const int64_t i0 = t * kMxTileElts + lane * 8;
    uint32_t lo, hi, s;
    mx_load_tile<kPlain>(wire + t * kMxTileBytes, lane, lo, hi, s);
    float v[8];
    mx_decode8(lo, hi, s, v);
    mx_store8<T, kPlain>(dst + i0 * (int64_t)sizeof(T), count - i0, vec, v);
  }
}

}  // namespace vccl
