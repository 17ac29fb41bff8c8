// The two main loops of the bf16x3 gather GEMMs: the kernels whose fp32 operand is gathered through per-row buffer descriptors and split (split2) in the
// kernel.  A kernel keeps its tile coordinates, its gather or load closure and its epilogue; the loop, the operand layout in LDS and the product live here, and so
// does what the planners and launchers share.  (Not conv_x3p.hip's conv_x3g_kernel, the pipelined k = 1 GEMM.)  Private to csrc/.
// conv_x3d_kernel and conv_flow_bwd_kernel (whose operand element is a function of three fetched values: gather_image_loop_act) run the image loop and
// conv_gen_wgrad_kernel the pair loop.  conv_x3d_bwd_kernel, conv_gen_bwd_kernel (image) and conv_x3d_wgrad_kernel (pair)
// still write their loop out around gather_mfma3_unit: called through the loops below they compute the same bits, but the compiler emits the address arithmetic
// in another order and they measured 0.6 - 1.8 % slower (profiles/x3g_dedup_isa.txt, x3g_dedup_timing.txt).  A change to a loop here is made there as well.
// conv_flow_wgrad_kernel (pair) writes its loop out too: its B operand holds two fetched values per element (WN's gate is formed between the load and the split).
//
// The product of one 16-deep unit and accumulator is three v_mfma_f32_32x32x16_bf16 in the order hi lo, lo hi, hi hi; a 32 x 32 accumulator holds column
// lane & 31 and rows acc_row32(r, lane >> 5).
//
// "image" (conv_x3d.hip, conv_x3d_bwd.hip, conv_gen_bwd.hip, conv_flow_bwd.hip): A is a weight image [unit][hi | lo][half][rows][8 ch] (x3_weight_image) and comes by LDS-DMA,
//   wave w fetching block (plane, half) = w of the unit in AR / 64 pieces of 1 KiB; B is gathered as fp32, wave w holding channels 4 w .. 4 w + 3 of the unit's
//   16-channel chunk at columns lane (+ 64), and is stored as [hi | lo][half][BN columns][8 ch].  LDS holds two slots of U units, a unit being its A block
//   (AR x 64 bytes) followed by its B block (BN x 64 bytes): stage st + 1 is fetched while stage st is multiplied, and a stage is what one barrier publishes,
//   so the latency of the fetch is paid once per U units (the grids of the deep layers are below one workgroup per CU: nothing else hides it).
// "pair" (conv_x3d_wgrad.hip, conv_gen_wgrad.hip): BOTH operands are fp32.  A stage is kKB = 128 reduction columns as kKU = 8 units; a load instruction fetches
//   ONE row of A or ONE column of B for 64 lanes, lane l holding the neighbours 2 l and 2 l + 1 of the stage, so a split2 gives one packed bf16 pair per plane
//   and the tiles [hi | lo][unit][half][row][8 k] are written with 32-bit LDS stores.  One LDS buffer; registers hold the next stage's loads while the current
//   one is multiplied.  The reduction is split over blockIdx.z into partial images that a finishing kernel adds in index order (gather_splits).
#pragma once
#include <algorithm>
#include "conv_x3_dev.h"

namespace rvc {

// row of element r of a 32 x 32 accumulator in the lane half lh = lane >> 5
__host__ __device__ constexpr int acc_row32(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// one unit: acc[am] += ah bl, += al bh, += ah bh, with ah / al at wa (+ alo) + 512 am and bh / bl at xa (+ blo)
template <int AM>
__device__ __forceinline__ void gather_mfma3_unit(f32x16 (&acc)[AM], const unsigned char* wa, int alo, const unsigned char* xa, int blo) {
  u32x4 ah[AM], al[AM];
#pragma unroll
  for (int am = 0; am < AM; ++am) {
    ah[am] = *reinterpret_cast<const u32x4*>(wa + am * 512);
    al[am] = *reinterpret_cast<const u32x4*>(wa + alo + am * 512);
  }
  const u32x4 bh = *reinterpret_cast<const u32x4*>(xa), bl = *reinterpret_cast<const u32x4*>(xa + blo);
#pragma unroll
  for (int am = 0; am < AM; ++am)
    acc[am] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[am]), __builtin_bit_cast(bf16x8, bl), acc[am], 0, 0, 0);
#pragma unroll
  for (int am = 0; am < AM; ++am)
    acc[am] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al[am]), __builtin_bit_cast(bf16x8, bh), acc[am], 0, 0, 0);
#pragma unroll
  for (int am = 0; am < AM; ++am)
    acc[am] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[am]), __builtin_bit_cast(bf16x8, bh), acc[am], 0, 0, 0);
}

// The image loop.  AR: rows of the A block (>= 64), BN: columns of the tile (CN = BN / 64 column groups), AM: accumulators per wave (rows 32 AM wm .. of the A
// block, columns 32 wn .. of the B block), U: units per stage.  ars / avoff / astep: the image's descriptor, this lane's byte offset in unit 0 and the bytes of
// one unit.  NV: fp32 values fetched per operand element.  gather(c, raw): called once per issued unit and column group c, in issue order; fills raw[v][i] with
// value v of this wave's four channels i at column 64 c + lane (out of range: zero, by the descriptor) and advances the closure's own (chunk, tap) after the
// unit's last group.  finish(c, raw, x): called in the same order when the stage's loads have landed, just before the split; x[i] = the operand element (a
// function of its NV fetched values: conv_flow_bwd.hip's gate derivative).  Zeroes and fills acc.
template <int AR, int BN, int AM, int U, int NV, class G, class F>
__device__ __forceinline__ void gather_image_loop_act(unsigned char* smem, __amdgpu_buffer_rsrc_t ars, int avoff, int astep, int nstages, int wave, int lane, int wm,
                                                      int wn, f32x16 (&acc)[AM], G gather, F finish) {
  constexpr int CN = BN / 64;
  constexpr int kASlot = AR * 64;              // bytes of [hi | lo][half][AR rows][16 B]
  constexpr int kBSlot = BN * 64;              // bytes of [hi | lo][half][BN columns][16 B]
  constexpr int kUSlot = kASlot + kBSlot, kSlot = U * kUSlot;
  const int li = lane & 31, lh = lane >> 5;

  float xr[U][CN][NV][4];
  int asoff = 0;                                                    // image offset of the next unit to be issued
  auto issue = [&](int slot) {
#pragma unroll
    for (int q = 0; q < U; ++q) {
      unsigned char* base = smem + slot * kSlot + q * kUSlot;
#pragma unroll
      for (int h = 0; h < AR / 64; ++h) buf_dma(ars, base + wave * (AR * 16) + h * 1024, avoff + h * 1024, asoff);
      asoff += astep;
#pragma unroll
      for (int c = 0; c < CN; ++c) gather(c, xr[q][c]);
    }
  };
  auto store_b = [&](int slot) {
    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int q = 0; q < U; ++q)
#pragma unroll
      for (int c = 0; c < CN; ++c) {
        float x[4];
        finish(c, xr[q][c], x);
        unsigned h0, l0, h1, l1;
        split2(x[0], x[1], h0, l0);
        split2(x[2], x[3], h1, l1);
        const u32x2_t hi = {h0, h1}, lo = {l0, l1};
        unsigned char* b = smem + slot * kSlot + q * kUSlot + kASlot + ((wave >> 1) * BN + c * 64 + lane) * 16 + (wave & 1) * 8;
        *reinterpret_cast<u32x2_t*>(b) = hi;
        *reinterpret_cast<u32x2_t*>(b + BN * 32) = lo;
      }
  };

#pragma unroll
  for (int am = 0; am < AM; ++am)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[am][r] = 0.f;

  issue(0);
  wait_vmcnt<0>();
  store_b(0);
  __syncthreads();

  const int aoff = (lh * AR + wm * (AM * 32) + li) * 16;
  const int boff = kASlot + (lh * BN + wn * 32 + li) * 16;
  for (int st = 0; st < nstages; ++st) {
    const int cur = st & 1;
    const bool more = st + 1 < nstages;
    if (more) issue(cur ^ 1);                    // slot cur ^ 1 was last read before the barrier that ended stage st - 1
#pragma unroll
    for (int q = 0; q < U; ++q) gather_mfma3_unit<AM>(acc, smem + cur * kSlot + q * kUSlot + aoff, AR * 32, smem + cur * kSlot + q * kUSlot + boff, BN * 32);
    if (more) {
      wait_vmcnt<0>();                           // this wave's weight pieces have landed in LDS, its gathered values in registers
      store_b(cur ^ 1);
    }
    __syncthreads();
  }
}
// the plain operand: one value per element, gather(c, x) fills this wave's four channel values
template <int AR, int BN, int AM, int U, class G>
__device__ __forceinline__ void gather_image_loop(unsigned char* smem, __amdgpu_buffer_rsrc_t ars, int avoff, int astep, int nstages, int wave, int lane, int wm,
                                                  int wn, f32x16 (&acc)[AM], G gather) {
  gather_image_loop_act<AR, BN, AM, U, 1>(smem, ars, avoff, astep, nstages, wave, lane, wm, wn, acc,
                                          [&](int c, float (&raw)[1][4]) { gather(c, raw[0]); },
                                          [](int, const float (&raw)[1][4], float (&x)[4]) {
#pragma unroll
                                            for (int i = 0; i < 4; ++i) x[i] = raw[0][i];
                                          });
}

// The pair loop.  BM x BN: the tile; a wave fetches BM / 4 rows of A and BN / 4 columns of B per stage and multiplies AM accumulators (rows 32 AM wm .., columns
// 32 wn ..).  Stages [g0, g1).  load(g, ar, br): fills this wave's rows and columns of stage g, element [i][h] being neighbour 2 lane + h of row / column
// (BM or BN) / 4 wave + i (out of range: zero).  actA / actB: applied to every value before the split.  Zeroes and fills acc.
constexpr int kGatherKB = 128, kGatherKU = kGatherKB / 16;
// one (unit, half) block of rows is padded by one 16-B row: the 16 groups of 4 lanes of a store land in 16 different bank quads
__host__ __device__ constexpr int gather_pair_block(int rows) { return rows * 16 + 16; }
template <int BM, int BN, int AM, class L, class FA, class FB>
__device__ __forceinline__ void gather_pair_loop(unsigned char* smem, int g0, int g1, int wave, int lane, int wm, int wn, f32x16 (&acc)[AM], L load, FA actA,
                                                 FB actB) {
  constexpr int kKU = kGatherKU, kARows = BM / 4, kBCols = BN / 4;
  constexpr int kABlock = gather_pair_block(BM), kBBlock = gather_pair_block(BN);
  constexpr int kAPlane = 2 * kKU * kABlock, kBPlane = 2 * kKU * kBBlock;
  const int li = lane & 31, lh = lane >> 5;

  float ar[kARows][2], br[kBCols][2];
  // lane l's pair is k = 2 l, 2 l + 1 of the stage: unit l >> 3, half (l >> 2) & 1, bytes 4 (l & 3) .. of the row's 16
  const int soff = (lane & 3) * 4;
  auto store = [&]() {
    unsigned char* a = smem + (lane >> 2) * kABlock + (wave * kARows) * 16 + soff;
#pragma unroll
    for (int i = 0; i < kARows; ++i) {
      unsigned hi, lo;
      split2(actA(ar[i][0]), actA(ar[i][1]), hi, lo);
      *reinterpret_cast<unsigned*>(a + i * 16) = hi;
      *reinterpret_cast<unsigned*>(a + i * 16 + kAPlane) = lo;
    }
    unsigned char* b = smem + 2 * kAPlane + (lane >> 2) * kBBlock + (wave * kBCols) * 16 + soff;
#pragma unroll
    for (int i = 0; i < kBCols; ++i) {
      unsigned hi, lo;
      split2(actB(br[i][0]), actB(br[i][1]), hi, lo);
      *reinterpret_cast<unsigned*>(b + i * 16) = hi;
      *reinterpret_cast<unsigned*>(b + i * 16 + kBPlane) = lo;
    }
  };

#pragma unroll
  for (int am = 0; am < AM; ++am)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[am][r] = 0.f;

  const int aoff = lh * kABlock + (wm * (AM * 32) + li) * 16;
  const int boff = 2 * kAPlane + lh * kBBlock + (wn * 32 + li) * 16;
  if (g0 < g1) load(g0, ar, br);
  for (int g = g0; g < g1; ++g) {
    __syncthreads();                               // the previous stage's operands have been read
    store();
    __syncthreads();
    if (g + 1 < g1) load(g + 1, ar, br);           // in flight while this stage is multiplied
#pragma unroll
    for (int ku = 0; ku < kKU; ++ku) gather_mfma3_unit<AM>(acc, smem + aoff + ku * 2 * kABlock, kAPlane, smem + boff + ku * 2 * kBBlock, kBPlane);
  }
}
struct GatherIdentity { __device__ __forceinline__ float operator()(float v) const { return v; } };
// the leaky ReLU as max(v, slope v): right for 0 <= slope <= 1 only (slope 1: none)
struct GatherLrelu { float slope; __device__ __forceinline__ float operator()(float v) const { return fmaxf(v, v * slope); } };

// ------------------------------------------------------------------------------------------------ host side: what the planners and launchers share
// units per stage: the largest of 4, 2, 1 that divides the unit count
inline int gather_units(long long nunits) { int u = 4; while (nunits % u) u >>= 1; return u; }
constexpr size_t gather_image_lds(int ar, int bn, int units) { return (size_t)2 * units * ((size_t)ar * 64 + (size_t)bn * 64); }
constexpr size_t gather_pair_lds(int bm, int bn) { return (size_t)4 * kGatherKU * ((size_t)gather_pair_block(bm) + (size_t)gather_pair_block(bn)); }
// The split count of a weight-gradient launch of `tiles` output tiles over `total` stages: about `target` workgroups, at most max_splits partial images, no split
// without a stage.  Returns the splits and sets per, the stages of one split.
inline int gather_splits(long long tiles, int total, long long target, long long max_splits, int& per) {
  const long long splits = std::min<long long>(std::min<long long>((target + tiles - 1) / tiles, max_splits), total);
  per = (int)((total + splits - 1) / splits);
  return (int)((total + per - 1) / per);
}
// f(std::integral_constant<int, U>) for the plan's units
template <class F> inline void gather_dispatch_units(int units, F&& f) {
  if (units == 4) f(std::integral_constant<int, 4>{});
  else if (units == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 1>{});
}

}  // namespace rvc
