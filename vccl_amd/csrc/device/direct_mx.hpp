// Two-shot direct all-reduce whose wire format is MXFP8 (mxfp8.hpp, DESIGN.md
// §4.19): ncclSum over f16 / bf16, opt-in (VCCL_AR_MXFP8_THRESHOLD).  The
// phases, flags, epochs and parities are direct_allreduce_part's (direct.hpp);
// what crosses a link is 33/32 bytes per element instead of 2:
//
//   out = narrow_T( D(E( D(E(x_0)) + D(E(x_1)) + ... + D(E(x_{n-1})) )) )
//
// every + a binary32 add in ascending rank order, E / D the codec, the second
// E on the binary32 sums, narrow_T the native RN-even narrowing, once.  Every
// contribution passes through the format, the owner's own included, and the
// owner stores to its own output what its peers decode: all ranks hold the
// same bits, whatever the shard ownership, chunking or block count.
//
// Geometry (host/plan.cc direct_mx_plan): everything is whole wire tiles of
// 512 elements.  A chunk of cc elements holds ceil(cc / 512) tiles, shard o
// the tiles [o * shardTiles, (o + 1) * shardTiles), shardTiles = ceil(tiles /
// n); chunk lengths are multiples of 512 n except the last, so codec blocks
// fall on global multiples of 32.  Workgroup b handles tiles [b * blkTiles,
// (b + 1) * blkTiles) of every shard (DirectWork::blkElts = 512 blkTiles); tile
// t of a shard sits at byte 528 t of a region, so workgroup b only ever touches
// the region bytes [528 b blkTiles, 528 (b + 1) blkTiles): the per-block flags
// order all reuse, as in every other direct kernel.  Wave w of the workgroup
// takes the block's tiles w, w + 8, ...: one tile per wave and step.
//   phase 1 (scatter): my input's tiles of every foreign shard p, encoded in
//            registers, straight into p's region (0, me): no staging buffer;
//   phase 2 (fold):    after direct_wait(0): per tile of my shard the n - 1
//            inbox tiles are loaded first, then decoded and added in rank
//            order, my own span encoded and decoded in registers at its place;
//            the sums are encoded, the wire tile stored to every peer's region
//            (1, me), its decoded, narrowed values to my own output;
//   phase 3 (gather):  after direct_wait(1): the owners' tiles from my inbox,
//            decoded and narrowed into my output.
// Chunk c + 1's scatter is issued after chunk c's fold and before its gather.
// Reuse: one epoch position per chunk; (1, *) regions and flags are written
// after direct_wait(0) of the chunk (R1), the gather's direct_wait(1) closes it
// (R2), parity p is rewritten for chunk c + 2 only after chunk c's readers'
// flags were awaited — the all-reduce's line of the proof in direct.hpp.
// User buffers off 16-byte alignment (or a short last span) take the element
// path of mx_load8 / mx_store8: alignment is local to a rank and steers
// nothing else.  In place: every element is read before the same lane, or a
// later phase, writes it.
#pragma once
#include "direct.hpp"
#include "mxfp8.hpp"

namespace vccl {

template <typename T>
__device__ void direct_allreduce_mx_part(const DirectWork& w, uint32_t& e, int& shFail) {
  constexpr int64_t esz = (int64_t)sizeof(T);
  const DirectPeers& P = *w.peers;
  const int n = w.nRanks, me = w.rank, b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
  char* myBuf = P.buf[me];
  const char* myFlags = P.flags[me];
  const int64_t blkTiles = w.blkElts / kMxTileElts;
  const int64_t inOff = (int64_t)b * blkTiles * kMxTileBytes;  // block offset in a region
  const bool inVec = ((uintptr_t)w.sendbuff & 15) == 0, outVec = ((uintptr_t)w.recvbuff & 15) == 0;

  auto chunk_geom = [&](int c, int64_t* c0, int64_t* cc, int64_t* shardTiles) {
    *c0 = (int64_t)c * w.chunkElts;
    const int64_t rest = (int64_t)w.count - *c0;
    *cc = rest < w.chunkElts ? rest : w.chunkElts;
    *shardTiles = ((*cc + kMxTileElts - 1) / kMxTileElts + n - 1) / n;
  };
  // block b of shard o: its first tile (chunk-relative) and its tile count
  auto block_of = [&](int64_t cc, int64_t shardTiles, int o, int64_t* t0, int64_t* nT) {
    const int64_t tiles = (cc + kMxTileElts - 1) / kMxTileElts;
    int64_t shardEnd = (int64_t)(o + 1) * shardTiles;
    shardEnd = shardEnd < tiles ? shardEnd : tiles;
    const int64_t lo = (int64_t)o * shardTiles + (int64_t)b * blkTiles;
    const int64_t hi = lo + blkTiles < shardEnd ? lo + blkTiles : shardEnd;
    *t0 = lo;
    *nT = hi > lo ? hi - lo : 0;
  };
  // Phase 1 (peer order rotated by the workgroup index, as the native scatter).
  auto scatter = [&](int c) {
    int64_t c0, cc, shardTiles;
    chunk_geom(c, &c0, &cc, &shardTiles);
    const char* in = (const char*)w.sendbuff + c0 * esz;
    for (int i = 0; i < n - 1; i++) {
      const int k = 1 + (b + i) % (n - 1);
      const int p = me + k < n ? me + k : me + k - n;
      int64_t t0, nT;
      block_of(cc, shardTiles, p, &t0, &nT);
      char* dst = P.buf[p] + direct_region_off(0, c & 1, me, n, w.regionBytes) + inOff;
      for (int64_t t = wv; t < nT; t += nw) {
        const int64_t i0 = (t0 + t) * kMxTileElts + lane * 8;
        float v[8];
        mx_load8<T, kSys>(in + i0 * esz, cc - i0, inVec, v);
        uint32_t lo, hi, s;
        mx_encode8(v, lo, hi, s);
        mx_store_tile<kSys>(dst + t * kMxTileBytes, lane, lo, hi, s);
      }
    }
  };

  if (w.nChunks <= 0) return;
  uint32_t eCur = epoch_after(e);
  if (!shFail) {
    scatter(0);
    direct_post(w, P, 0, 0, b, eCur);
  }
  for (int c = 0; c < w.nChunks; c++) {
    const int par = c & 1;
    const uint32_t eNext = epoch_after(eCur);
    int64_t c0, cc, shardTiles;
    chunk_geom(c, &c0, &cc, &shardTiles);
    const char* in = (const char*)w.sendbuff + c0 * esz;
    char* out = (char*)w.recvbuff + c0 * esz;
    // Phase 2: fold my shard's block b, send the wire tiles out, keep their decoded values.
    if (!shFail && direct_wait(w, myFlags, 0, par, b, eCur, &shFail)) {
      int64_t t0, nT;
      block_of(cc, shardTiles, me, &t0, &nT);
      for (int64_t t = wv; t < nT; t += nw) {
        const int64_t i0 = (t0 + t) * kMxTileElts + lane * 8;
        const int64_t wOff = inOff + t * kMxTileBytes;
        uint32_t lo[kDirectMaxRanks], hi[kDirectMaxRanks], s[kDirectMaxRanks];
        // every inbox tile's loads are issued before the first decode; the arrays are indexed by unrolled
        // constants only (registers), my own tile is kept beside them and selected by q == me
#pragma unroll
        for (int q = 0; q < kDirectMaxRanks; q++) {
          lo[q] = hi[q] = s[q] = 0;
          if (q < n && q != me)
            mx_load_tile<kSys>(myBuf + direct_region_off(0, par, q, n, w.regionBytes) + wOff, lane, lo[q], hi[q], s[q]);
        }
        float x[8];
        mx_load8<T, kSys>(in + i0 * esz, cc - i0, inVec, x);
        uint32_t mlo, mhi, ms;
        mx_encode8(x, mlo, mhi, ms);
        float acc[8];
        mx_decode8(me == 0 ? mlo : lo[0], me == 0 ? mhi : hi[0], me == 0 ? ms : s[0], acc);
#pragma unroll
        for (int q = 1; q < kDirectMaxRanks; q++) {
          if (q < n) {
            float v[8];
            mx_decode8(q == me ? mlo : lo[q], q == me ? mhi : hi[q], q == me ? ms : s[q], v);
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] += v[j];
          }
        }
        uint32_t rlo, rhi, rs;
        mx_encode8(acc, rlo, rhi, rs);
#pragma unroll
        for (int j = 0; j < kDirectMaxRanks - 1; j++) {
          if (j < n - 1) {
            const int dst = me + j + 1 < n ? me + j + 1 : me + j + 1 - n;
            mx_store_tile<kSys>(P.buf[dst] + direct_region_off(1, par, me, n, w.regionBytes) + wOff, lane, rlo, rhi,
                                rs);
          }
        }
        mx_decode8(rlo, rhi, rs, acc);
        mx_store8<T, kSys>(out + i0 * esz, cc - i0, outVec, acc);
      }
    }
    if (!shFail) direct_post(w, P, 1, par, b, eCur);
    // Chunk c+1's scatter before chunk c's gather.
    if (c + 1 < w.nChunks && !shFail) {
      scatter(c + 1);
      direct_post(w, P, 0, par ^ 1, b, eNext);
    }
    // Phase 3: decode the other owners' tiles into my output.
    if (!shFail && direct_wait(w, myFlags, 1, par, b, eCur, &shFail)) {
      for (int k = 1; k < n; k++) {
        const int o = me + k < n ? me + k : me + k - n;
        int64_t t0, nT;
        block_of(cc, shardTiles, o, &t0, &nT);
        const char* src = myBuf + direct_region_off(1, par, o, n, w.regionBytes) + inOff;
        for (int64_t t = wv; t < nT; t += nw) {
          const int64_t i0 = (t0 + t) * kMxTileElts + lane * 8;
          uint32_t lo, hi, s;
          mx_load_tile<kSys>(src + t * kMxTileBytes, lane, lo, hi, s);
          float v[8];
          mx_decode8(lo, hi, s, v);
          mx_store8<T, kSys>(out + i0 * esz, cc - i0, outVec, v);
        }
      }
    }
    __syncthreads();  // this chunk's region reads precede later posts
    e = eCur;
    eCur = eNext;
  }
}

// A batch of such calls (DirectBatch, as direct_batch runs the native parts): one epoch sequence, retired once.
template <typename T>
__device__ __forceinline__ void direct_batch_mx(const DirectBatch& bt) {
  __shared__ int shFail;
  const DirectWork& w = bt.w;
  uint32_t e = __hip_atomic_load(&w.comm->dEpoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x == 0) shFail = 0;
  __syncthreads();
  // one call site: the part function is inlined once
  for (int i = 0; i < bt.nParts; i++)
    direct_allreduce_mx_part<T>(i ? direct_work_with(w, bt.more[i - 1]) : w, e, shFail);
  epoch_retire(&w.comm->dEpoch, &w.comm->dDone, e);
}

// ------------------------------------------- reduce-scatter and all-gather
// The one-hop direct reduce-scatter and all-gather in the format (DESIGN.md
// §4.20; opt-in, VCCL_RSAG_MXFP8_THRESHOLD), ncclSum over f16 / bf16 and f16 /
// bf16 blocks.  w.count = c, the per-rank count in elements:
//
//   reduce-scatter, rank p:  out[j] = narrow_T( D(E(x_0[p c ..)))[j] + ... + D(E(x_{n-1}[p c ..)))[j] )
//   all-gather, every rank:  out[r c + j] = narrow_T( D(E(x_r))[j] )
//
// every + a binary32 add in ascending rank order, the owner's / sender's own
// contribution through the format too, one narrowing, no second quantization.
// Codec blocks are cut by the index j WITHIN one rank's block of c elements.
//
// Geometry (host/plan.cc direct_mx_rsag_plan): a chunk is a range of one
// rank's block, whole wire tiles except the call's last; workgroup b handles
// the chunk's tiles [b * blkTiles, (b + 1) * blkTiles), tile t of them at byte
// 528 (b * blkTiles + t) of a region, wave w the tiles w, w + 8, ...  Flags,
// epochs, the region (0, me) of parity 0 and the three phases with the closing
// acknowledgement are direct_reducescatter_part's / direct_allgather_part's
// (direct.hpp), and so is their reuse argument: a peer overwrites my region
// only after my phase-3 acknowledgement.  A short last tile crosses the link
// as a whole wire tile, its missing elements 0; they never reach user memory.
// The 16-byte path of mx_load8 / mx_store8 is chosen per pointer: rank p's
// block starts at p * c elements, off 16 bytes whenever c is odd.
template <typename T>
__device__ void direct_reducescatter_mx_part(const DirectWork& w, uint32_t& e, int& shFail) {
  constexpr int64_t esz = (int64_t)sizeof(T);
  const DirectPeers& P = *w.peers;
  const int n = w.nRanks, me = w.rank, b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int64_t count = (int64_t)w.count;
  const char* myBuf = P.buf[me];
  const char* myFlags = P.flags[me];
  const int64_t blkTiles = w.blkElts / kMxTileElts;
  const int64_t inOff = (int64_t)b * blkTiles * kMxTileBytes;  // block offset in a region
  for (int c = 0; c < w.nChunks; c++) {
    e = epoch_after(e);
    if (shFail) continue;
    const int64_t c0 = (int64_t)c * w.chunkElts;
    const int64_t cc = count - c0 < w.chunkElts ? count - c0 : w.chunkElts;
    const int64_t tiles = (cc + kMxTileElts - 1) / kMxTileElts, t0 = (int64_t)b * blkTiles;
    const int64_t tEnd = t0 + blkTiles < tiles ? t0 + blkTiles : tiles;
    const int64_t nT = tEnd > t0 ? tEnd - t0 : 0;  // my block's tiles of this chunk
    // Phase 1: my contribution to every foreign owner's block, encoded in registers, straight into its inbox
    // (workgroup b starts at peer offset 1 + b mod (n - 1), as the native scatter).
    for (int i = 0; i < n - 1; i++) {
      const int k = 1 + (b + i) % (n - 1);
      const int p = me + k < n ? me + k : me + k - n;
      const char* src = (const char*)w.sendbuff + ((int64_t)p * count + c0) * esz;
      const bool vec = ((uintptr_t)src & 15) == 0;
      char* dst = P.buf[p] + direct_region_off(0, 0, me, n, w.regionBytes) + inOff;
      for (int64_t t = wv; t < nT; t += nw) {
        const int64_t i0 = (t0 + t) * kMxTileElts + lane * 8;
        float v[8];
        mx_load8<T, kSys>(src + i0 * esz, cc - i0, vec, v);
        uint32_t lo, hi, s;
        mx_encode8(v, lo, hi, s);
        mx_store_tile<kSys>(dst + t * kMxTileBytes, lane, lo, hi, s);
      }
    }
    direct_post(w, P, 0, 0, b, e);
    // Phase 2: fold my block in rank order, my own span through the format in registers; one narrowing.
    if (direct_wait(w, myFlags, 0, 0, b, e, &shFail)) {
      const char* mine = (const char*)w.sendbuff + ((int64_t)me * count + c0) * esz;
      char* out = (char*)w.recvbuff + c0 * esz;
      const bool inVec = ((uintptr_t)mine & 15) == 0, outVec = ((uintptr_t)out & 15) == 0;
      for (int64_t t = wv; t < nT; t += nw) {
        const int64_t i0 = (t0 + t) * kMxTileElts + lane * 8;
        const int64_t wOff = inOff + t * kMxTileBytes;
        uint32_t lo[kDirectMaxRanks], hi[kDirectMaxRanks], s[kDirectMaxRanks];
        // every inbox tile's loads are issued before the first decode (arrays indexed by unrolled constants)
#pragma unroll
        for (int q = 0; q < kDirectMaxRanks; q++) {
          lo[q] = hi[q] = s[q] = 0;
          if (q < n && q != me)
            mx_load_tile<kSys>(myBuf + direct_region_off(0, 0, q, n, w.regionBytes) + wOff, lane, lo[q], hi[q], s[q]);
        }
        float x[8];
        mx_load8<T, kSys>(mine + i0 * esz, cc - i0, inVec, x);
        uint32_t mlo, mhi, ms;
        mx_encode8(x, mlo, mhi, ms);
        float acc[8];
        mx_decode8(me == 0 ? mlo : lo[0], me == 0 ? mhi : hi[0], me == 0 ? ms : s[0], acc);
#pragma unroll
        for (int q = 1; q < kDirectMaxRanks; q++) {
          if (q < n) {
            float v[8];
            mx_decode8(q == me ? mlo : lo[q], q == me ? mhi : hi[q], q == me ? ms : s[q], v);
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] += v[j];
          }
        }
        mx_store8<T, kSys>(out + i0 * esz, cc - i0, outVec, acc);
      }
    }
    direct_post(w, P, 1, 0, b, e);
    // Phase 3: the peers' acknowledgements for this chunk.
    (void)direct_wait(w, myFlags, 1, 0, b, e, &shFail);
  }
}

template <typename T>
__device__ void direct_allgather_mx_part(const DirectWork& w, uint32_t& e, int& shFail) {
  constexpr int64_t esz = (int64_t)sizeof(T);
  const DirectPeers& P = *w.peers;
  const int n = w.nRanks, me = w.rank, b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int64_t count = (int64_t)w.count;
  const char* myBuf = P.buf[me];
  const char* myFlags = P.flags[me];
  const int64_t blkTiles = w.blkElts / kMxTileElts;
  const int64_t inOff = (int64_t)b * blkTiles * kMxTileBytes;  // block offset in a region
  for (int c = 0; c < w.nChunks; c++) {
    e = epoch_after(e);
    if (shFail) continue;
    const int64_t c0 = (int64_t)c * w.chunkElts;
    const int64_t cc = count - c0 < w.chunkElts ? count - c0 : w.chunkElts;
    const int64_t tiles = (cc + kMxTileElts - 1) / kMxTileElts, t0 = (int64_t)b * blkTiles;
    const int64_t tEnd = t0 + blkTiles < tiles ? t0 + blkTiles : tiles;
    const int64_t nT = tEnd > t0 ? tEnd - t0 : 0;
    // Phase 1: one load and one encode per tile; the wire tile to every peer, what they will decode to my own
    // block of the output (in place: this lane has read the 8 elements it now writes).
    {
      const char* src = (const char*)w.sendbuff + c0 * esz;
      char* own = (char*)w.recvbuff + ((int64_t)me * count + c0) * esz;
      const bool inVec = ((uintptr_t)src & 15) == 0, ownVec = ((uintptr_t)own & 15) == 0;
      const size_t rOff = direct_region_off(0, 0, me, n, w.regionBytes) + inOff;
      for (int64_t t = wv; t < nT; t += nw) {
        const int64_t i0 = (t0 + t) * kMxTileElts + lane * 8;
        float v[8];
        mx_load8<T, kSys>(src + i0 * esz, cc - i0, inVec, v);
        uint32_t lo, hi, s;
        mx_encode8(v, lo, hi, s);
#pragma unroll
        for (int j = 0; j < kDirectMaxRanks - 1; j++) {
          if (j < n - 1) {
            const int p = me + j + 1 < n ? me + j + 1 : me + j + 1 - n;
            mx_store_tile<kSys>(P.buf[p] + rOff + t * kMxTileBytes, lane, lo, hi, s);
          }
        }
        mx_decode8(lo, hi, s, v);
        mx_store8<T, kSys>(own + i0 * esz, cc - i0, ownVec, v);
      }
    }
    direct_post(w, P, 0, 0, b, e);
    // Phase 2: the other ranks' tiles from my inbox, decoded and narrowed into their blocks of the output.
    if (direct_wait(w, myFlags, 0, 0, b, e, &shFail)) {
      for (int k = 1; k < n; k++) {
        const int o = me + k < n ? me + k : me + k - n;
        const char* src = myBuf + direct_region_off(0, 0, o, n, w.regionBytes) + inOff;
        char* dst = (char*)w.recvbuff + ((int64_t)o * count + c0) * esz;
        const bool vec = ((uintptr_t)dst & 15) == 0;
        for (int64_t t = wv; t < nT; t += nw) {
          const int64_t i0 = (t0 + t) * kMxTileElts + lane * 8;
          uint32_t lo, hi, s;
          mx_load_tile<kSys>(src + t * kMxTileBytes, lane, lo, hi, s);
          float v[8];
          mx_decode8(lo, hi, s, v);
          mx_store8<T, kSys>(dst + i0 * esz, cc - i0, vec, v);
        }
      }
    }
    direct_post(w, P, 1, 0, b, e);
    // Phase 3: the peers' acknowledgements for this chunk.
    (void)direct_wait(w, myFlags, 1, 0, b, e, &shFail);
  }
}

// A batch of such calls of one collective (AG: the all-gather), as direct_batch_mx runs the all-reduces.
template <typename T, bool AG>
__device__ __forceinline__ void direct_batch_mx_rsag(const DirectBatch& bt) {
  __shared__ int shFail;
  const DirectWork& w = bt.w;
  uint32_t e = __hip_atomic_load(&w.comm->dEpoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x == 0) shFail = 0;
  __syncthreads();
  for (int i = 0; i < bt.nParts; i++) {
    const DirectWork wi = i ? direct_work_with(w, bt.more[i - 1]) : w;
    if constexpr (AG) direct_allgather_mx_part<T>(wi, e, shFail);
    else direct_reducescatter_mx_part<T>(wi, e, shFail);
  }
  epoch_retire(&w.comm->dEpoch, &w.comm->dDone, e);
}

}  // namespace vccl
