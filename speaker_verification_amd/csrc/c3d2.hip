// The C3D2 embedding network's first three blocks (model.py:110-131, :141-164).
//   c3d2_stage1h_kernel   cube + conv1_1 + conv1_2 + pool1 on v_mfma_f32_16x16x32_f16 through two-piece f16 products (round 4)
//   c3d2_conv21h_kernel   conv2_1, two-piece f16 products
//   c3d2_conv22h_kernel   conv2_2 + pool2, two-piece f16 products
//   c3d2_conv31h_kernel   conv3_1, two-piece f16 products; writes the chunked, column-major layout c3d2_conv32h_kernel stages
//   c3d2_conv32h_kernel   conv3_2, two-piece f16 products, K split over two waves per N tile
//   c3d2_conv41h_kernel   conv4_1, two-piece f16 products; writes the chunked layout c3d2_conv42_kernel stages
// (conv4_2 and FC5, on the f32 matrix pipe, are in c3d2_tail.hip; the leaf helpers of all of them in c3d2_common.h.)  BatchNorm
// (eval mode) is folded into weights and biases by the host (model.FusedEmbedder).  Work items come from device-wide counters.
// What earlier rounds built and superseded is
// under tools/experiments/ with its measured numbers: the direct-form f32 kernels, the t-plane first block, the K-split conv3_2
// (c3d2_superseded_r3.patch) and the f32 first and second blocks through the depth transform, round 4's 7.12 + 5.09 ms kernels
// (stage1_f32_winograd.patch, stage2_f32_winograd.patch).
//
// The first block as ONE gfx950 kernel:
//   feature rows + crop starts -> cube (utils.py:351-379) -> conv1_1 (1 -> 16, k(3,1,5)) + BN + PReLU
//   -> conv1_2 (16 -> 16, k(3,9,1), stride (1,2,1)) + BN + PReLU -> MaxPool3d((1,1,2))
// (/root/reference/model.py:110-117 and :141-150).  These two layers are 46 % of the network's multiply-adds, and
// conv1_1's output is the network's largest tensor (3.3 MB per cube); here it only ever exists as a 100 KB tile in LDS.
//
// Work item = (cube u, pooled output column j, half q of the output depths): conv1_2 outputs
//   d in [8q, 8q + 8), h in [0, 36), w in {2j, 2j + 1}  ->  pooled column j, 16 channels.
// A persistent workgroup of 8 waves (two per SIMD; it owns the CU's LDS) loops over items; the kernel is the item loop over four
// phases, each a function of its own below:
//   1. convert_patch: the 12 x 80 x 6 cube patch the item needs is moved into LDS by LDS-DMA (dma_patch_w) inside the previous
//      item's matrix work and converted in place to (h, l) half pairs by the waves that fetched it;
//   2. conv11_one_channel / conv11_three_channels: conv1_1 as a GEMM [16 channels] x [K = 32: 15 taps + pad, h | l] x [16 pixels]
//      (conv11_mfma), + PReLU, split into (h, l), written to the act1 tile in LDS (park_pieces): 10 depths x 80 rows x 2 columns x
//      16 channels;
//   3. conv12_chain / conv12_tile: conv1_2 as an implicit GEMM in the direct form, two taps per K = 32 block, the weights of all 27
//      taps in 112 VGPRs; a wave walks one set of 16 (row, column) positions along the depth and reads every fragment (Conv12Frags)
//      once for its three kd (depth chains);
//   4. prelu_pool_store: bias (in the accumulator), PReLU, max over the column pair (adjacent lanes: one DPP instruction), 16-byte
//      stores.
// Barriers, waits and the item pipeline are in the kernel itself (conv11_three_channels owns the two barriers around its staged
// channels).  The other kernels of this file are one function each; all share the leaf helpers of c3d2_common.h, and the host side
// one parameter struct (ConvParams), one set of argument checks (conv_checks) and one entry body (conv_entry).
#include <climits>
#include <vector>

#include "c3d2_common.h"
#include "svk_internal.h"

namespace {

constexpr int NCROP = 20, NFRAME = 80, NCOEF = 40;  // cube geometry (utils.py:20-21)
constexpr int TD = 8;                                // conv1_2 output depths per item
constexpr int DIN = TD + 2;                          // act1 depths per item
constexpr int PD = TD + 4;                           // cube patch depths per item
constexpr int OD = 16, OH = 36, OWP = 18;            // output: depths, rows, pooled columns
// output strides (floats) of [n][16 d][36 h][18 w][16 c] (channels-last memory of a (n, 16, 16, 36, 18) tensor): pooled column,
// row parity, depth, cube.  Compile-time: as kernel parameters they were 64-bit scalar multiplies per item
constexpr int S_W = 16, S_PAR = OWP * 16, S_D = OH * OWP * 16, S_N = OD * OH * OWP * 16;
// A work item (cube u, rem = 18 q + j: half q of the output depths, pooled column j), decoded ONCE when its index is known (two
// items ahead) and handed down: item / 36, % 36, / 18 for the item, the next one (patch fetch) and the one after (crop starts)
// were three division chains of scalar instructions per item, in front of the barrier where nothing hides them.
// NJ = the LIVE pooled columns of the launch, a cube's items being 2 NJ: 18, or 17 where the caller hands the output to the second
// block only (flags bit 5; see stage1 below).  The 17-column form numbers a cube's items 17 q + j and decodes them to the SAME
// rem = 18 q + j, j <= 16, so everything behind the decode -- patch, tiles, output strides -- is the 18-column kernel's; NJ is
// compile-time for the reason S_W is (the divisor).
struct ItemPos {
  int u, rem;
  __device__ __forceinline__ int q() const { return rem >= 18 ? 1 : 0; }
  __device__ __forceinline__ int j() const { return rem >= 18 ? rem - 18 : rem; }
  template <int NJ>
  __device__ static __forceinline__ ItemPos of(int item) {
    static_assert(NJ == OWP || NJ == OWP - 1, "18 live columns, or 17");
    const int u = item / (2 * NJ), r = item - 2 * NJ * u;
    if constexpr (NJ == OWP) return ItemPos{u, r};
    else return ItemPos{u, r >= NJ ? r + (OWP - NJ) : r};
  }
};

struct Stage1Params {
  const float* feat;
  const int32_t* crop;
  int32_t n_utt, max_frames;
  const u32x4* w1blk;    // [2][64]: conv1_1's A blocks (8 halves per lane): [H taps 0-15 | H taps 0-15], [L taps 0-15 | 0]
  const float* bias1;
  const float* slope1;
  const u32x4* w2blk;    // [14 pairs][2][64]: [H_a | H_b], [L_a | L_b]; lane (co = l & 15, kk): ci = 8 (kk & 1) + e, tap a (kk < 2) / b;
                         // pair 13 (one tap): [H_a | H_a], [L_a | 0]
  const float* bias2;
  const float* slope2;
  float* out;
  unsigned* queue;
  int32_t cubes_per_clip;   // the *_multi entries (MULTI instances of the kernel) only: cube u reads the feature rows of clip u / K
};

// a per-thread constant plus an immediate.
// (a VECTOR load by lanes 0 .. 11, not twelve scalar loads: scalar loads return out of order, so while any is in
// flight every LDS wait of the wave becomes lgkmcnt(0) -- the first gather read of the conv1_1 phase then stalled for
// the crop table's whole L2 round trip, 2 500 cycles per item by the in-kernel stamps)
__device__ __forceinline__ int fetch_starts(const Stage1Params& p, ItemPos it, int lane) {
  const int32_t* cr = p.crop + (int64_t)it.u * NCROP + TD * it.q();
  return cr[lane < PD ? lane : 0];
}

constexpr int WPW = 8;                                     // floats per patch row in LDS: [ww 0 1 2 | - | ww 3 4 5 | -]
constexpr int WP_FLOATS = PD * NFRAME * WPW;               // 7 680

// The item's cube patch by LDS-DMA (global_load_lds_dwordx3; round 3): patch[dd][h][.] = feat[u][crop[u][8 q + dd] + h][2 j ..
// 2 j + 5].  A DMA lane's 12 bytes land at a wave-uniform LDS base + 16 lane (measured: tools/experiments/glds12_probe.hip
// -- the fourth word of every 16 bytes is left alone), so two lanes carry a row's two halves, the row is 8 floats in LDS
// and one instruction moves 32 rows: no staging registers, no parking writes, no per-lane address arithmetic (the register
// path before it: twelve 8-byte loads + six ds_write_b64 per thread).  The source needs 4-byte alignment only.  Depth
// dd's 80 rows are three pieces (32 + 32 + 16 rows, the last with half the lanes).
// WHO fetches matters more than how: the workgroup's four OLDER waves (part 0) finish their tiles ~5 k cycles before the
// younger four and wait at the item's last barrier, so they carry the whole fetch -- nine pieces each: depths pair, pair + 4,
// pair + 8, the piece's part a compile-time constant -- and the younger waves, whose tiles end the item, none: the
// scalar address work and the issue of a fetch spread over all eight waves cost 2.5 % of the kernel (7.70 -> 7.51 ms; a
// build with no fetch at all: 7.33).  A piece that is not wholly inside the clip (a wild crop start: the C-ABI takes any
// int32) goes the slow way, lane by lane, with zeros outside -- a wave-uniform branch the pipeline's own crops never take.
struct PatchPiece { const float* src; float* dst; int rows; bool inside; int start, h0; };
__device__ __forceinline__ void patch_piece_issue(const Stage1Params& p, const PatchPiece& pc, int lane) {
  const int rl = lane >> 1, half = lane & 1;
  if (pc.inside) {
    if (rl < pc.rows) __builtin_amdgcn_global_load_lds(pc.src + rl * NCOEF + 3 * half, pc.dst, 12, 0, 0);
  } else if (rl < pc.rows) {
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if ((unsigned)pc.start < (unsigned)p.max_frames && pc.h0 + rl < p.max_frames - pc.start) {
      const float* src = pc.src + rl * NCOEF + 3 * half;
      v0 = src[0];
      v1 = src[1];
      v2 = src[2];
    }
    float* d = pc.dst + rl * WPW + 4 * half;
    d[0] = v0;
    d[1] = v1;
    d[2] = v2;
  }
}
// the nine pieces of wave `pair` (a part-0 wave).  Every crop start is read BEFORE the first DMA: with one in flight the
// compiler drains vmcnt in front of any use of an ordinary load's result -- `starts_v` is one -- which would serialise them.
__device__ __forceinline__ void dma_patch_w(const Stage1Params& p, ItemPos it, int starts_v, int pair, int lane, float* patch) {
  const float* base = p.feat + (int64_t)it.u * ((int64_t)p.max_frames * NCOEF) + 2 * it.j();
  int st[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) st[g] = __builtin_amdgcn_readlane(starts_v, pair + 4 * g);
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int part = 0; part < 3; ++part) {
      PatchPiece pc;
      pc.rows = part < 2 ? 32 : 16;
      pc.h0 = 32 * part;
      pc.start = st[g];
      pc.dst = patch + ((pair + 4 * g) * NFRAME + pc.h0) * WPW;
      pc.inside = (unsigned)st[g] < (unsigned)p.max_frames && pc.h0 + pc.rows <= p.max_frames - st[g];   // (cannot overflow for any int32 start)
      pc.src = base + (int64_t)(st[g] + pc.h0) * NCOEF;
      patch_piece_issue(p, pc, lane);
    }
}
// the same for the item's feature matrix `plane` of a layout with several per cube: channel c of cube u is plane 3 u + c in the
// three-channel layout [n][3][max_frames][40]
__device__ __forceinline__ void dma_patch_plane(const Stage1Params& p, ItemPos it, int64_t plane, int starts_v, int pair, int lane,
                                                float* patch) {
  Stage1Params q = p;
  q.feat = p.feat + (plane - it.u) * ((int64_t)p.max_frames * NCOEF);
  dma_patch_w(q, it, starts_v, pair, lane, patch);
}

// =====================================================================================================
// The first block on the F16 matrix pipe through TWO-PIECE products (round 4, second half).  An f32 value x is carried as
// the pair (h, l) of halves with h = f16(x), l = f16(x - h): 22 significant bits in the same four bytes, and
//     x w  =  h_x h_w + l_x h_w + h_x l_w      (+ l_x l_w, 2^-22 of the product: dropped)
// is three f16 products, exact in the f32 the MFMA accumulates in.  Measured on this network's layers (CPU emulation with
// the trained checkpoint): 0.9 - 4.6e-7 of the activation scale from the f64 convolution -- the f32 direct form itself is
// 1.8 - 7.9e-7 (its error is the accumulation's).  `v_mfma_f32_16x16x32_f16` issues every 16 cycles with K = 32: 16 x the
// multiply-adds per cycle of `v_mfma_f32_16x16x4_f32`, so three piece products cost 3 / 16 of one f32 product, and
//   * the pieces are made where a value is PRODUCED (conv1_1's epilogue: 2.5 vector instructions per value with
//     v_cvt_pk_f16_f32; the patch is converted in place once per item), never at a fragment read;
//   * the depth transform is gone (its adds do not distribute over pieces): the direct form's 27 taps, two taps per K = 32
//     block -- [h_a | h_b] x [H_a | H_b],  [l_a | l_b] x [H_a | H_b],  [h_a | h_b] x [L_a | L_b] -- 42 MFMAs of 16 cycles per
//     tile of 16 output positions where the f32 kernel issues 144 of 32;
//   * act1 = 64 bytes per pixel as before, as FOUR planes of 16-byte slots (h c0-7, h c8-15, l c0-7, l c8-15), each split by
//     the parity of the row: slot ((quarter * 2 + (r & 1)) * 10 + dd) * 80 + (r >> 1) * 2 + col.  A B fragment is one
//     ds_read_b128, and the 16 positions of a tile (8 output rows x 2 columns, input rows 2 apart: one parity) are 16
//     CONSECUTIVE slots for every lane group of the LDS (the channel half and the tap of a K = 32 block pick planes, not
//     slots): conflict-free.  (Pixels as 64-byte records put eight rows of a tile on the same banks: 8-way conflicts.);
//   * a tile is ANY 16 positions (the operand address is per lane): the 576 positions of an item are 36 full tiles, no
//     remainder tiles, no exchange buffer.
// Same boundary as svk_c3d2_stage1 (f32 feature rows + crop starts in, f32 pooled activation out).
// =====================================================================================================
constexpr int HACT_WORDS = 16 * DIN * NFRAME * 2;            // 25 600 32-bit words = 6 400 slots of 16 bytes
constexpr int HPLANE = DIN * NFRAME;                         // slots per (quarter, row parity) plane: [10 dd][40 r / 2][2 col]
constexpr int HPAIRS = 14;                                   // tap pairs of conv1_2 (27 taps + one empty)

// conv1_1's K order.  A B fragment is four patch words, each the (h, l) pair of one tap's value as the conversion leaves it
// (low half h, high half l): K = 8 kk + 2 e + {0: h, 1: l}, so the A operand is [H_t | H_t] x 4 and [L_t | 0] x 4 -- the three
// piece products of the 15 taps in two MFMAs, as before, but a lane reads four words where the [h | h | l | l] order read eight
// and sorted their halves with four v_perm_b32.  The taps (kd, kw), t = 5 kd + kw, are cut into dominoes that ONE read
// instruction can fetch for every lane: words 0, 1 of a lane = a vertical pair (kd, kw), (kd + 1, kw), one depth = 640 words
// apart (ds_read2st64_b32); words 2, 3 = a horizontal pair (kd, kw), (kd, kw + 1) with kw in {0, 3}, adjacent words in a row
// [c0 c1 c2 - | c3 c4 c5 -] for both column parities:
//   kk = 0: (0-1, 1), (2; 0-1)    kk = 1: (0-1, 2), (0; 3-4)    kk = 2: (0-1, 0), (1; 3-4)    kk = 3: (1-2, 2), (2; 3-4)
// Tap (1, 2) lies in two dominoes; kk = 3's copy takes tap 15's zero weight.
constexpr unsigned long long CONV11_TAPS = 0xedcf98504372ba61ull;   // t of word e of lane group kk: 4 bits at 4 (4 kk + e)
__device__ __forceinline__ int conv11_tap(int kk, int e) { return (int)(CONV11_TAPS >> (4 * (4 * kk + e))) & 15; }
// the word offset of word e of lane group kk (e = 0: its vertical pair, e = 2: its horizontal pair) from pixel (dd, r, c)'s row
__device__ __forceinline__ int conv11_word(int kk, int e, int c) {
  const int t = conv11_tap(kk, e), kd = t == 15 ? 1 : t / 5, col = c + (t == 15 ? 2 : t % 5);
  return kd * (NFRAME * WPW) + col + (col >= 3 ? 1 : 0);
}
// A = [H_t | H_t], [L_t | 0] for the four taps of lane (i, kk), gathered from a d_w1blk block in svk.h's order: element (lane
// co + 16 (t >> 3), e = t & 7) is tap t of output channel co, H in the block's first 64 lanes, L in its second (t = 15 is 0)
__device__ __forceinline__ void conv11_weights(const unsigned short* blk, int i, int kk, u32x4& WH, u32x4& WL) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int t = conv11_tap(kk, e), x = (i + 16 * (t >> 3)) * 8 + (t & 7);
    const unsigned h = blk[x], l = blk[64 * 8 + x];
    WH[e] = h | (h << 16);
    WL[e] = l;
  }
}

// The three-channel first block (svk_c3d2_stage1_c3; utils.FeatureCube3C, model.py:110 with num_channels = 3) is the same kernel
// with NCH = 3: feature rows [n][3][max_frames][40], conv1_1's K = 45 taps as three K = 32 blocks [h | l] of one channel's 15 taps
// + a zero tap each (six MFMAs per tile instead of two), the accumulators of a wave's 13 tiles kept in registers across the three
// channel passes.  Channel 0 comes through the patch buffer as before (fetched inside the previous item's conv1_2); channels 1
// and 2 are fetched at the top of the item into the act1 tile, which is free until conv1_1's epilogue writes it, while channel 0
// is multiplied.  conv1_2, the pool and the output layout are the one-channel kernel's.  (The two differ in their conv1_1 phase,
// conv11_one_channel / conv11_three_channels, and in conv1_2's walk: see the kernel.)
// conv1_2's depth chains (conv12_chain): CONV12_CHAIN output depths per chain; its units in issue order are the four
// pair units of input depth s = 0 .. CONV12_CHAIN + 1 and, behind those of every s >= 2, pairs 12 and 13 of output s - 2
constexpr int CONV12_CHAIN = 4, CONV12_UNITS = 4 * (CONV12_CHAIN + 2) + 2 * CONV12_CHAIN;
constexpr int conv12_unit_step(int n) { return n < 8 ? n / 4 : 2 + (n - 8) / 6; }
constexpr int conv12_unit_sub(int n) { return n < 8 ? n % 4 : (n - 8) % 6; }   // 0 .. 3: pair m of the step; 4, 5: pairs 12, 13
static_assert(2 * CONV12_CHAIN == TD, "two chains cover an item's output depths");

// Where an item's feature rows lie: the item with u = the CLIP its cube reads -- the cube itself, or cube / K for the K cubes per
// clip of svk_c3d2_stage1_multi / svk_c3d2_stage1_c3_multi (a MULTI instance of the kernel: the one-cube-per-clip instances carry
// no division).  dma_patch_w and dma_patch_plane form the row base from it (plane = 3 clip + c); the crop table and the output
// stay indexed by the cube.
template <bool MULTI>
__device__ __forceinline__ ItemPos feat_pos(const Stage1Params& p, ItemPos it) {
  if constexpr (MULTI) it.u = (int)((unsigned)it.u / (unsigned)p.cubes_per_clip);
  return it;
}

// A lane's place in the workgroup of eight waves: lane = 16 kk + i, wave = 4 part + pair (wave-uniform).  Part 0 are the four
// OLDER waves, which fetch and convert the patches (see dma_patch_w)
struct Lane1 { int lane, wave, i, kk, pair, part; };

// the item's channel-0 patch (the one-channel kernel's only one): plane NCH u of [n][NCH][max_frames][40]
template <int NCH, bool MULTI>
__device__ __forceinline__ void dma_patch_ch0(const Stage1Params& p, ItemPos it, int starts_v, const Lane1& L, float* patch) {
  const ItemPos src = feat_pos<MULTI>(p, it);
  if constexpr (NCH == 1) dma_patch_w(p, src, starts_v, L.pair, L.lane, patch);
  else dma_patch_plane(p, src, (int64_t)NCH * src.u, starts_v, L.pair, L.lane, patch);
}

// ---- phase 1: the patch at `buf` in place, f32 -> (l << 16 | h) words: by the wave that FETCHED the words (its own vmcnt(0) is
// all it needs: no barrier of its own), depths pair, pair + 4, pair + 8 = 3 x 640 words = nine 16-byte trips per lane, all nine
// reads in flight before the first conversion.  (As a pass of all eight waves in front of conv1_1, behind a barrier: 0.45 of 4.11 ms.)
__device__ __forceinline__ void convert_patch(float* buf, int pair, int lane) {
  f32x4 v[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int w = (pair + 4 * (k / 3)) * (NFRAME * WPW) + 256 * (k % 3) + 4 * lane;
    if (k % 3 < 2 || lane < 32) v[k] = *reinterpret_cast<const f32x4*>(buf + w);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int w = (pair + 4 * (k / 3)) * (NFRAME * WPW) + 256 * (k % 3) + 4 * lane;
    unsigned h0, l0, h1, l1;
    split2(__builtin_shufflevector(v[k], v[k], 0, 1), h0, l0);
    split2(__builtin_shufflevector(v[k], v[k], 2, 3), h1, l1);
    u32x4 o;   // word = the value's own pair: low half h, high half l
    o[0] = __builtin_amdgcn_perm(l0, h0, 0x05040100u);
    o[1] = __builtin_amdgcn_perm(l0, h0, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(l1, h1, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(l1, h1, 0x07060302u);
    if (k % 3 < 2 || lane < 32) *reinterpret_cast<u32x4*>(buf + w) = o;
  }
}

// ---- phase 2: conv1_1 + PReLU -> act1 as (h, l): 100 tiles of 16 pixels, tile tt = wave + 8 m (m = 12: waves 0 - 3 only) ----
// A lane's addresses.  Its B fragment is four patch words, each a tap's (h, l) pair as it lies in the patch (K order: conv11_tap):
// the vertical pair at pov and the horizontal pair at poh, patch-word offsets of tile m = 0 (pixel 16 tt + i of tile tt: row
// 8 tt + (i >> 1)); tile m is 64 rows on
__device__ __forceinline__ int conv11_patch_word(const Lane1& L, int e) { return (8 * L.wave + (L.i >> 1)) * WPW + conv11_word(L.kk, e, L.i & 1); }
// pixel 16 tt + i = (dd = tt / 10, r = 8 (tt % 10) + (i >> 1), col = i & 1): slot 8 tt + 2 (i >> 2) + (i & 1) of the plane
// (quarter kk >> 1 [+ 2 for l], parity (i >> 1) & 1); the lane's four channels are bytes 8 (kk & 1) .. + 7 of the slot.  -> the
// h words of tile m = 0; tile m is 4 * 64 m words on, the l words 4 * 4 * HPLANE
__device__ __forceinline__ unsigned* conv11_act_word(unsigned* act, const Lane1& L) {
  return act + 4 * ((((L.kk >> 1) * 2 + ((L.i >> 1) & 1)) * HPLANE) + 8 * L.wave + 2 * (L.i >> 2) + (L.i & 1)) + 2 * (L.kk & 1);
}
__device__ __forceinline__ u32x4 conv11_frag(const unsigned* pv, const unsigned* ph, int m) {
  const int o = 64 * WPW * m;
  return (u32x4){pv[o], pv[o + NFRAME * WPW], ph[o], ph[o + 1]};
}
// one channel's K = 32 block, A = (WH, WL), into the accumulators of tiles m0 .. m0 + NT - 1: acc[t] = (FIRST ? bias : acc[t]) + ..
template <bool FIRST, int NT>
__device__ __forceinline__ void conv11_mfma(const unsigned* pv, const unsigned* ph, int m0, u32x4 WH, u32x4 WL, f32x4 bias, f32x4* acc) {
  u32x4 B[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    B[t] = conv11_frag(pv, ph, m0 + t);
    // (a fence per tile: without it the compiler pairs words of DIFFERENT tiles into one read2 and reassembles B with
    // three v_mov_b32 per tile)
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, WH), __builtin_bit_cast(f16x8, B[t]), FIRST ? bias : acc[t], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < NT; ++t)
    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, WL), __builtin_bit_cast(f16x8, B[t]), acc[t], 0, 0, 0);
}
// NT tiles from the patch to act1
template <bool SLOPE01, int NT>
__device__ __forceinline__ void conv11_tiles(const unsigned* pv, const unsigned* ph, unsigned* aw, int m0, u32x4 WH, u32x4 WL, f32x4 bias, f32x4 slope) {
  f32x4 acc[NT];
  conv11_mfma<true, NT>(pv, ph, m0, WH, WL, bias, acc);
#pragma unroll
  for (int t = 0; t < NT; ++t) park_pieces(aw + 4 * 64 * (m0 + t), 4 * 4 * HPLANE, prelu4<SLOPE01>(acc[t], slope), true);
}
template <bool SLOPE01>
__device__ __forceinline__ void conv11_one_channel(const unsigned* patch, int pov, int poh, unsigned* aw, const Lane1& L, u32x4 WH, u32x4 WL,
                                                   f32x4 bias, f32x4 slope) {
#pragma unroll
  for (int m0 = 0; m0 < 12; m0 += 4) conv11_tiles<SLOPE01, 4>(patch + pov, patch + poh, aw, m0, WH, WL, bias, slope);
  if (L.wave < 4) conv11_tiles<SLOPE01, 1>(patch + pov, patch + poh, aw, 12, WH, WL, bias, slope);
}
// one channel's K = 32 block (its patch at `src`) into the accumulators of the wave's 13 tiles (the bias rides in with channel 0)
template <bool FIRST>
__device__ __forceinline__ void conv11_chan_pass(const unsigned* src, int pov, int poh, const Lane1& L, u32x4 WH, u32x4 WL, f32x4 bias,
                                                 f32x4 (&acc)[13]) {
#pragma unroll
  for (int m0 = 0; m0 < 12; m0 += 2) conv11_mfma<FIRST, 2>(src + pov, src + poh, m0, WH, WL, bias, acc + m0);
  if (L.wave < 4) conv11_mfma<FIRST, 1>(src + pov, src + poh, 12, WH, WL, bias, acc + 12);
}
// The three-channel form, with its two barriers: channel 0 from the patch buffer; channels 1 and 2 of this item -> the act1 tile's
// first 2 x 30 KB (nobody reads act1 between the last item's final barrier and this item's epilogue), by the waves that fetch
// channel 0; they land while channel 0 is multiplied
template <bool SLOPE01, int NCH, bool MULTI>
__device__ __forceinline__ void conv11_three_channels(const Stage1Params& p, ItemPos cur, int starts_cur, unsigned* act, const float* patch,
                                                      int pov, int poh, unsigned* aw, const Lane1& L, f32x4 bias, f32x4 slope) {
  float* const chan12 = reinterpret_cast<float*>(act);
  if (L.part == 0) {
    const ItemPos src = feat_pos<MULTI>(p, cur);
#pragma unroll
    for (int ch = 1; ch < NCH; ++ch)
      dma_patch_plane(p, src, (int64_t)NCH * src.u + ch, starts_cur, L.pair, L.lane, chan12 + (ch - 1) * WP_FLOATS);
  }
  f32x4 acc[13];   // tile wave + 8 m; m = 12 for waves 0 - 3 only
  // conv1_1's weight blocks are gathered per item (L1-resident, 16 halves per lane per channel): held across the item loop as
  // W1a / W1b are in the one-channel kernel, the six blocks and the 13 accumulators spill (256 VGPRs).  The opaque copy of the pointer
  // keeps the compiler from hoisting the loads out of the loop.
  const unsigned short* w1blk = reinterpret_cast<const unsigned short*>(p.w1blk);
  asm volatile("" : "+s"(w1blk));
  {
    u32x4 WH, WL;
    conv11_weights(w1blk, L.i, L.kk, WH, WL);
    conv11_chan_pass<true>(reinterpret_cast<const unsigned*>(patch), pov, poh, L, WH, WL, bias, acc);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of channels 1 and 2 have landed
  if (L.part == 0) {
#pragma unroll
    for (int ch = 1; ch < NCH; ++ch) convert_patch(chan12 + (ch - 1) * WP_FLOATS, L.pair, L.lane);
  }
  __syncthreads();   // channels 1 and 2 are in place and converted
#pragma unroll
  for (int ch = 1; ch < NCH; ++ch) {
    u32x4 WH, WL;
    conv11_weights(w1blk + 2 * ch * 64 * 8, L.i, L.kk, WH, WL);
    conv11_chan_pass<false>(reinterpret_cast<const unsigned*>(chan12 + (ch - 1) * WP_FLOATS), pov, poh, L, WH, WL, bias, acc);
  }
  __syncthreads();   // every wave has read channels 1 and 2: act1 may be written
#pragma unroll
  for (int m = 0; m < 13; ++m) {
    if (m == 12 && L.wave >= 4) break;
    park_pieces(aw + 4 * 64 * m, 4 * 4 * HPLANE, prelu4<SLOPE01>(acc[m], slope), true);
  }
}

// ---- phases 3 and 4: conv1_2 + PReLU + pool: 576 positions (depth, row, column) in tiles of 16 ----
// The B fragments of the 16 positions (depth d + .., row, column i & 1) a lane group reads.  Pixel (dd, r = 2 row + kh, col),
// channels 8 (kk & 1) .. + 7: slot (((kk & 1) * 2 + (kh & 1)) * 10 + dd) * 80 + (row + kh / 2) * 2 + col of the h planes; the l
// planes 4 HPLANE slots on.  The taps of a pair (kd, 2 m), (kd, 2 m + 1) differ by the parity plane (a2); the pair 12 = (0, 8) |
// (1, 8) by one depth (a3); pair 13 = the LAST tap (2, 8) alone, as [h | l] in ONE fragment (a13: lanes kk >= 2 read the l planes):
// [H | H] x [h | l] + [L | 0] x [h | l] are its three piece products in two MFMAs and one read, where [h | -] and [l | -] against
// [H | 0], [L | 0] were three and two
struct Conv12Frags {
  const char *a2, *a3, *a13;
  __device__ __forceinline__ Conv12Frags(const unsigned* act, int d, int row, int i, int kk) {
    const int base = 16 * (((kk & 1) * 2) * HPLANE + d * 80 + 2 * row + (i & 1));
    a2 = reinterpret_cast<const char*>(act) + base + (kk >= 2 ? 16 * HPLANE : 0);
    a3 = reinterpret_cast<const char*>(act) + base + (kk >= 2 ? 16 * 80 : 0);
    a13 = a3 + (kk >= 2 ? 16 * 4 * HPLANE - 16 * 80 : 0);
  }
  // piece (0: h, 1: l) of pair m < 4 at INPUT depth d + dd (any kd: the fragment depends on the input depth alone), or of pair 12
  // (m = 4) / pair 13 (m = 5) of OUTPUT depth d + dd
  __device__ __forceinline__ u32x4 rd(int dd, int m, int piece) const {
    const char* ad = m < 4 ? a2 + 1280 * dd + 32 * m : m == 4 ? a3 + 1280 * dd + 32 * 4 : a13 + 1280 * (dd + 2) + 32 * 4;
    return *reinterpret_cast<const u32x4*>(ad + 16 * 4 * HPLANE * piece);
  }
};
// pair pr's piece products: three, two for the last pair (its fragment is [h | l]: no l fragment)
__device__ __forceinline__ f32x4 conv12_pieces(const u32x4 (&W2)[HPAIRS][2], int pr, u32x4 h, u32x4 l, f32x4 c) {
  return mfma_pieces(W2[pr][0], W2[pr][1], h, l, c, pr < HPAIRS - 1);
}

// One stand-alone tile: 16 positions (dq, row, column i & 1), every fragment read by the tile itself (27 reads, 41 MFMAs):
// pair pr: 0 .. 11 = (kd = pr / 4, kh = 2 (pr % 4) | + 1), then 12 and 13
template <bool SLOPE01>
__device__ __forceinline__ void conv12_tile(const unsigned* act, const u32x4 (&W2)[HPAIRS][2], f32x4 bias, f32x4 slope, float* obase,
                                            int dq, int row, const Lane1& L) {
  const Conv12Frags f(act, dq, row, L.i, L.kk);
  auto rd = [&](int pr, int piece) -> u32x4 { return pr < 12 ? f.rd(pr / 4, pr % 4, piece) : f.rd(0, pr - 8, piece); };
  f32x4 acc = bias;
  // fragments TWO pairs ahead (three rotating sets): a pair is 48 cycles of MFMA, less than an LDS round trip
  u32x4 bh[3], bl[3];
  bh[0] = rd(0, 0);
  bl[0] = rd(0, 1);
  bh[1] = rd(1, 0);
  bl[1] = rd(1, 1);
#pragma unroll
  for (int pr = 0; pr < HPAIRS; ++pr) {
    if (pr + 2 < HPAIRS) {
      bh[(pr + 2) % 3] = rd(pr + 2, 0);
      if (pr + 2 < HPAIRS - 1) bl[(pr + 2) % 3] = rd(pr + 2, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    acc = conv12_pieces(W2, pr, bh[pr % 3], bl[pr % 3], acc);
    __builtin_amdgcn_sched_barrier(0);
  }
  prelu_pool_store<SLOPE01>(acc, slope, obase + dq * S_D + row * S_PAR, (L.i & 1) == 0);
}

// A DEPTH CHAIN: the fragment of pair (kd, m) of output (dq, row, col) is the act1 slot of (dq + kd, row + m, col) -- it
// depends on the input depth dq + kd alone, so a wave that keeps ONE set of 16 (row, col) positions over consecutive
// output depths reads the eight fragments (pairs m = 0 .. 3, h and l) of an input depth ONCE and multiplies them into
// three live accumulators: kd = 0 of output dd, kd = 1 of dd - 1, kd = 2 of dd - 2.  An output whose kd = 2 step is done
// takes pairs 12 and 13 (three reads of its own) and leaves through the epilogue.  Every output receives its 41 MFMAs
// in the stand-alone tile's order (kd-major, pairs 0 - 3 inside a kd, then 12, 13) with the same operands: bit-identical.
// Eight chains of four output depths, one per wave: rows 8 pt .. 8 pt + 7 (pt = wave & 3) x depth half (wave >> 2), six
// input depths, 6 x 8 + 4 x 3 = 60 reads for 164 MFMAs.  Rows 32 - 35 (64 positions) are four stand-alone tiles of two
// depths each on the YOUNGER waves (the older ones fetch and convert the next patch): 588 reads per item, not 972.
template <bool SLOPE01>
__device__ __forceinline__ void conv12_chain(const unsigned* act, const u32x4 (&W2)[HPAIRS][2], f32x4 bias, f32x4 slope, float* obase,
                                             const Lane1& L) {
  const int row = 8 * L.pair + (L.i >> 1), d0 = 4 * L.part;
  const Conv12Frags f(act, d0, row, L.i, L.kk);
  // unit n of the chain's 32 (conv12_unit_step / _sub): the four pairs of input depth s, behind them (s >= 2) pairs 12
  // and 13 of output s - 2.  Fragments TWO units ahead, three rotating sets, as in the stand-alone tile
  auto rd = [&](int n, int piece) -> u32x4 {
    const int s = conv12_unit_step(n), e = conv12_unit_sub(n);
    return f.rd(e < 4 ? s : s - 2, e, piece);
  };
  f32x4 acc[CONV12_CHAIN];
  u32x4 bh[3], bl[3];
  bh[0] = rd(0, 0);
  bl[0] = rd(0, 1);
  bh[1] = rd(1, 0);
  bl[1] = rd(1, 1);
#pragma unroll
  for (int n = 0; n < CONV12_UNITS; ++n) {
    if (n + 2 < CONV12_UNITS) {
      bh[(n + 2) % 3] = rd(n + 2, 0);
      if (conv12_unit_sub(n + 2) != 5) bl[(n + 2) % 3] = rd(n + 2, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    const int s = conv12_unit_step(n), e = conv12_unit_sub(n);
    if (e < 4) {
#pragma unroll
      for (int kd = 0; kd < 3; ++kd) {
        const int o = s - kd;
        if (o >= 0 && o < CONV12_CHAIN) acc[o] = conv12_pieces(W2, 4 * kd + e, bh[n % 3], bl[n % 3], kd == 0 && e == 0 ? bias : acc[o]);
      }
    } else {
      const int o = s - 2;
      acc[o] = conv12_pieces(W2, 8 + e, bh[n % 3], bl[n % 3], acc[o]);
      if (e == 5) prelu_pool_store<SLOPE01>(acc[o], slope, obase + (d0 + o) * S_D + row * S_PAR, (L.i & 1) == 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The driver: the prologue (operands that stay in registers: conv1_2's weights, 112 VGPRs; NCH = 1: conv1_1's too), the first
// item's patch, then the item loop over phases 2 - 4 with phase 1 of the NEXT item inside.  Items: `item` is multiplied, item1's
// patch is fetched (crop starts: `starts`), item2's crop starts are fetched, item3 is drawn from the device-wide counter.
// (NCH = 3 keeps conv1_2's tile loop: with 13 conv1_1 accumulators behind it the chain takes its spill from 6 to 16 VGPRs)
// MULTI: p.n_utt counts CUBES, K = p.cubes_per_clip of them per clip's feature rows (feat_pos); nothing else differs.
// NJ: the live pooled columns (ItemPos): 2 NJ items per cube; with NJ = 17 nothing computes or writes column 17.
template <bool SLOPE01, int NCH = 1, bool MULTI = false, int NJ = OWP>
__global__ __launch_bounds__(512) void c3d2_stage1h_kernel(const Stage1Params p) {
  constexpr bool CONV12_CHAINS = NCH == 1;
  extern __shared__ __attribute__((aligned(16))) float smem_c3d2[];
  unsigned* const act = reinterpret_cast<unsigned*>(smem_c3d2);   // [HACT_WORDS]
  float* const patch = smem_c3d2 + HACT_WORDS;                    // [WP_FLOATS]: [12 dd][80 h][8], f32 from the DMA, then (l << 16 | h) words
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Lane1 L{lane, wave, lane & 15, lane >> 4, wave & 3, wave >> 2};
  const int n_items = p.n_utt * (2 * NJ);

  u32x4 W2[HPAIRS][2];
  load_wblk(p.w2blk, 0, lane, W2);
  u32x4 W1a, W1b;   // NCH = 1: conv1_1's A operand, held across the item loop (NCH = 3 gathers its three per item)
  if constexpr (NCH == 1) conv11_weights(reinterpret_cast<const unsigned short*>(p.w1blk), L.i, L.kk, W1a, W1b);
  const int pov = conv11_patch_word(L, 0), poh = conv11_patch_word(L, 2);
  f32x4 b1v, sl1v, b2v, sl2v;   // a lane holds channels 4 kk .. 4 kk + 3 of ONE position (A = the weights)
  load_bias_slope(p.bias1, p.slope1, 0, L.kk, b1v, sl1v);
  load_bias_slope(p.bias2, p.slope2, 0, L.kk, b2v, sl2v);

  int starts = 0;
  int starts_cur = 0;   // NCH = 3: the current item's crop starts (`starts` is already the next item's by the top of the loop)
  __shared__ int q_item3;
  int item = blockIdx.x, item1 = item + (int)gridDim.x, item2 = item1 + (int)gridDim.x;
  ItemPos cur = ItemPos::of<NJ>(item), nx = ItemPos::of<NJ>(item1), nx2 = ItemPos::of<NJ>(item2);
  if (item < n_items) {
    starts = fetch_starts(p, cur, lane);
    if (L.part == 0) dma_patch_ch0<NCH, MULTI>(p, cur, starts, L, patch);
    starts_cur = starts;
    if (item1 < n_items) starts = fetch_starts(p, nx, lane);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (L.part == 0 && item < n_items) convert_patch(patch, L.pair, lane);
  __syncthreads();
  while (item < n_items) {
    const int next = item1;
    unsigned q_ticket = 0;
    if (threadIdx.x == 0 && p.queue) q_ticket = atomicAdd(p.queue, 1u);

    // ---- conv1_1 + PReLU -> act1 ----
    unsigned* const aw = conv11_act_word(act, L);
    if constexpr (NCH == 1)
      conv11_one_channel<SLOPE01>(reinterpret_cast<const unsigned*>(patch), pov, poh, aw, L, W1a, W1b, b1v, sl1v);
    else
      conv11_three_channels<SLOPE01, NCH, MULTI>(p, cur, starts_cur, act, patch, pov, poh, aw, L, b1v, sl1v);
    if (threadIdx.x == 0) q_item3 = p.queue ? (int)q_ticket + 3 * (int)gridDim.x : item2 + (int)gridDim.x;
    __syncthreads();   // act1 is complete; the patch buffer is free
    const int item3 = q_item3;

    // ---- the next item's patch (it lands inside this item's conv1_2), the crop starts of the one after ----
    if (L.part == 0 && next < n_items) {
      dma_patch_ch0<NCH, MULTI>(p, nx, starts, L, patch);
      starts_cur = starts;
      if (item2 < n_items) starts = fetch_starts(p, nx2, lane);
    }
    // ---- conv1_2 + PReLU + pool -> out ----
    float* const obase = p.out + (int64_t)cur.u * S_N + (TD * cur.q()) * S_D + cur.j() * S_W + 4 * L.kk;
    if constexpr (CONV12_CHAINS) {
      conv12_chain<SLOPE01>(act, W2, b2v, sl2v, obase, L);
      if (L.part) conv12_tile<SLOPE01>(act, W2, b2v, sl2v, obase, 2 * L.pair + (L.i >> 3), 32 + ((L.i >> 1) & 3), L);
    } else {
      // tiles t = wave + 8 m (m < 4) of positions P = 16 t + i -> (depth P / 72, row, column); the last four go to the YOUNGER
      // waves (the older ones fetch and convert the next patch)
#pragma unroll 1
      for (int m = 0; m < 4 + L.part; ++m) {
        const int t = m < 4 ? wave + 8 * m : 28 + wave;
        const int P = 16 * t + L.i;
        const int dq = (P * 911) >> 16, rem = P - 72 * dq;          // P / 72 for P < 576
        conv12_tile<SLOPE01>(act, W2, b2v, sl2v, obase, dq, rem >> 1, L);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces have landed
    if (L.part == 0 && next < n_items) convert_patch(patch, L.pair, lane);
    __syncthreads();  // the next patch is in place and converted; act1 may be overwritten
    item = item1;
    item1 = item2;
    item2 = item3;
    cur = nx;
    nx = nx2;
    nx2 = ItemPos::of<NJ>(item3);
  }
}

// svk_c3d2_stage1 (NCH = 1) and svk_c3d2_stage1_c3 (NCH = 3): the same arguments, checks and launch.  Their *_multi forms
// (MULTI) take `n_clips` feature matrices and K = cubes_per_clip cubes of each: every check below then applies to the cube count
// n_clips K, which is what the kernel calls n_utt.
// flags: bit 1 (value 2) = every slope in [0, 1]; bit 5 (value 32) = the 17-column form: the caller hands d_out to svk_c3d2_stage2
// only, which reads pooled columns 0 .. 16 (conv2_1 is 4 wide and pool2 drops its 15th column), so column 17 is neither computed nor
// written.  The bits between them stay UNDEFINED, like 1: the tests pin 1, 4, 8 and 16 as SVK_ERR_BAD_ARG on these entries.
constexpr int32_t STAGE1_SLOPE01 = 2, STAGE1_LIVE17 = 32;
template <int NCH, bool MULTI = false>
int stage1(svk_ctx* ctx, const char* name, const float* d_feat, int32_t n_clips, int32_t max_frames, int32_t n_cols,
           const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, const void* d_w1blk, const float* d_bias1,
           const float* d_slope1, const void* d_w2blk, const float* d_bias2, const float* d_slope2, int32_t flags, float* d_out,
           int32_t cubes_per_clip = 1) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, (flags & ~(STAGE1_SLOPE01 | STAGE1_LIVE17)) == 0,
              "flags: only bit 1 (slopes in [0, 1]) and bit 5 (pooled column 17 left unwritten) are defined");
  SVK_REQUIRE(ctx, cubes_per_clip >= 1, "cubes_per_clip must be at least 1");
  SVK_REQUIRE(ctx, n_clips >= 0 && max_frames >= 1, "shape");
  SVK_REQUIRE(ctx, (int64_t)n_clips * cubes_per_clip <= INT32_MAX, "too many cubes for one launch");   // (the item count: below)
  const int32_t n_utt = n_clips * cubes_per_clip;
  if (n_cols != NCOEF || n_crops != NCROP || crop_frames != NFRAME)
    return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "%s is built for the %s20 x 80 x 40 cube of utils.py:%s (got %d x %d x %d)", name,
                    NCH == 3 ? "3 x " : "", NCH == 3 ? "325-348" : "20-21", n_crops, crop_frames, n_cols);
  if (n_utt == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_feat && d_crop_idx && d_w1blk && d_bias1 && d_slope1 && d_w2blk && d_bias2 && d_slope2 && d_out,
              "NULL buffer");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_feat) & 7) == 0 && ((reinterpret_cast<uintptr_t>(d_w1blk) | reinterpret_cast<uintptr_t>(d_w2blk) |
                                                                    reinterpret_cast<uintptr_t>(d_out)) & 15) == 0,
              "d_feat must be 8-byte, the weight blocks and d_out 16-byte aligned");
  // (36 items per cube: the 18-column count, the stricter bound for either form)
  SVK_REQUIRE(ctx, (int64_t)n_utt * 36 + 4 * (int64_t)ctx->num_cu < ((int64_t)1 << 31), "too many cubes for one launch");
  Stage1Params p;
  p.feat = d_feat;
  p.crop = d_crop_idx;
  p.n_utt = n_utt;
  p.max_frames = max_frames;
  p.w1blk = static_cast<const u32x4*>(d_w1blk);
  p.bias1 = d_bias1;
  p.slope1 = d_slope1;
  p.w2blk = static_cast<const u32x4*>(d_w2blk);
  p.bias2 = d_bias2;
  p.slope2 = d_slope2;
  p.out = d_out;
  p.cubes_per_clip = cubes_per_clip;
  const bool slope01 = flags & STAGE1_SLOPE01;
  const int live = (flags & STAGE1_LIVE17) ? OWP - 1 : OWP;
  void (*kern)(const Stage1Params) =
      live == OWP ? (slope01 ? c3d2_stage1h_kernel<true, NCH, MULTI, OWP> : c3d2_stage1h_kernel<false, NCH, MULTI, OWP>)
                  : (slope01 ? c3d2_stage1h_kernel<true, NCH, MULTI, OWP - 1> : c3d2_stage1h_kernel<false, NCH, MULTI, OWP - 1>);
  unsigned grid;
  if (int rc = svk_persistent_grid(ctx, name, kern, svk_c3d2_stage1_lds_bytes(), 512, 1, (int64_t)n_utt * 2 * live, &grid)) return rc;
  if (int rc = svk_work_queue(ctx, SVK_SLOT_STAGE1, 1, &p.queue)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), svk_c3d2_stage1_lds_bytes(), ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // namespace

extern "C" {

size_t svk_c3d2_stage1_lds_bytes(void) { return sizeof(float) * (size_t)(HACT_WORDS + WP_FLOATS); }
// channels 1 and 2 are staged inside the act1 tile: the one-channel kernel's footprint
static_assert((3 - 1) * WP_FLOATS <= HACT_WORDS, "the staged channels must fit in the act1 tile");
size_t svk_c3d2_stage1_c3_lds_bytes(void) { return svk_c3d2_stage1_lds_bytes(); }

int svk_c3d2_stage1(svk_ctx* ctx, const float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
                     const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, const void* d_w1blk,
                     const float* d_bias1, const float* d_slope1, const void* d_w2blk, const float* d_bias2,
                     const float* d_slope2, int32_t flags, float* d_out) {
  return stage1<1>(ctx, "svk_c3d2_stage1", d_feat, n_utt, max_frames, n_cols, d_crop_idx, n_crops, crop_frames, d_w1blk, d_bias1,
                   d_slope1, d_w2blk, d_bias2, d_slope2, flags, d_out);
}

int svk_c3d2_stage1_c3(svk_ctx* ctx, const float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
                       const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, const void* d_w1blk,
                       const float* d_bias1, const float* d_slope1, const void* d_w2blk, const float* d_bias2,
                       const float* d_slope2, int32_t flags, float* d_out) {
  return stage1<3>(ctx, "svk_c3d2_stage1_c3", d_feat, n_utt, max_frames, n_cols, d_crop_idx, n_crops, crop_frames, d_w1blk,
                   d_bias1, d_slope1, d_w2blk, d_bias2, d_slope2, flags, d_out);
}

int svk_c3d2_stage1_multi(svk_ctx* ctx, const float* d_feat, int32_t n_clips, int32_t max_frames, int32_t n_cols,
                          const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, const void* d_w1blk,
                          const float* d_bias1, const float* d_slope1, const void* d_w2blk, const float* d_bias2,
                          const float* d_slope2, int32_t flags, float* d_out, int32_t cubes_per_clip) {
  return stage1<1, true>(ctx, "svk_c3d2_stage1_multi", d_feat, n_clips, max_frames, n_cols, d_crop_idx, n_crops, crop_frames, d_w1blk,
                         d_bias1, d_slope1, d_w2blk, d_bias2, d_slope2, flags, d_out, cubes_per_clip);
}

int svk_c3d2_stage1_c3_multi(svk_ctx* ctx, const float* d_feat, int32_t n_clips, int32_t max_frames, int32_t n_cols,
                             const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, const void* d_w1blk,
                             const float* d_bias1, const float* d_slope1, const void* d_w2blk, const float* d_bias2,
                             const float* d_slope2, int32_t flags, float* d_out, int32_t cubes_per_clip) {
  return stage1<3, true>(ctx, "svk_c3d2_stage1_c3_multi", d_feat, n_clips, max_frames, n_cols, d_crop_idx, n_crops, crop_frames,
                         d_w1blk, d_bias1, d_slope1, d_w2blk, d_bias2, d_slope2, flags, d_out, cubes_per_clip);
}

}  // extern "C"

// =====================================================================================================
// The second block: conv2_1 (16 -> 32, kernel (3,1,4)) + BN + PReLU, conv2_2 (32 -> 32, kernel (3,8,1),
// stride (1,2,1)) + BN + PReLU + MaxPool3d((1,1,2))  (/root/reference/model.py:119-124, :151-158), two
// kernels of the same shape as the matrix phase above: the input region of a work item is staged in LDS
// as padded 'pixels' (one pixel = the channel vector of one (d, h, w) position), the weights of the
// wave's output-channel tile(s) sit in registers, and the A operand of every tap is one ds_read_b128
// at a fixed offset from the M tile's base address.
// =====================================================================================================
namespace {

// What every kernel below takes; each kernel's header comment gives its `in`, `wblk` and `out` layouts
struct ConvParams {
  const float* in;
  const u32x4* wblk;    // weight blocks [..][2: H | L][64 lanes] of eight halves
  const float* bias;    // [output channels]
  const float* slope;   // [output channels]
  float* out;
  int32_t n_utt;
  unsigned* queue;      // work-item counter (zeroed before the launch), or NULL: items at a fixed stride
};

constexpr int S2_D = 16, S2_H = 36, S2_W = 18;       // input of conv2_1 (after pool1), 16 channels
constexpr int A2_D = 14, A2_W = 14;                  // conv2_1 output (32 channels), rows = S2_H.  The layer has 15 columns; pool2 drops
                                                     // conv2_2's 15th, which is all that reads conv2_1's 15th (kernel width 1): never computed
constexpr int O2_D = 12, O2_H = 15, O2_W = 7;        // after conv2_2 + pool2 (32 channels)

// ---- conv2_1 through two-piece f16 products (see c3d2_stage1h_kernel): direct form, 12 taps = 6 pairs (kd, kw | kw + 1) of
// K = 32 blocks, three MFMAs per pair and N tile (both N tiles of a wave share the B fragments).  Item = (cube, block of 4
// rows) as before; its input [16 d][4 rows][18 w][16 c] is split into (h, l) while it is staged and lies in LDS as four planes
// of 16-byte slots (h c0-7, h c8-15, l c0-7, l c8-15), slot = pixel (d * 4 + row) * 18 + col: the 16 positions of a tile --
// ANY 16 consecutive outputs of the item's 14 d x 4 rows x 14 columns = 784 = 49 full tiles -- read consecutive slots (+ 4 across a
// row end).  36 MFMAs of 16 cycles per tile where the depth-transformed f32 kernel issued 128 of 32 per 16 positions of a pair.
//   in   [n][16][36][18][16]          out  [n][14][36][14][32]
//   wblk [2 nt][6 pairs][2][64]: lane (co = 16 nt + (l & 15), kk): e: W[co][8 (kk & 1) + e][kd][kw + (kk >= 2)], pair = 2 kd + kw / 2 ----
constexpr int C21H_PIX = S2_D * 4 * S2_W;            // 1 152 pixels = slots per plane
constexpr int C21H_LDS_WORDS = 4 * 4 * C21H_PIX;     // four planes of 16-byte slots: 73 728 bytes
constexpr int C21H_POS = A2_D * 4 * A2_W;            // 784 output positions per item

template <bool SLOPE01>
__global__ __launch_bounds__(256, 2) void c3d2_conv21h_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem_c21w[];
  unsigned* const reg = reinterpret_cast<unsigned*>(smem_c21w);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, kk = lane >> 4;
  u32x4 W[2][6][2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) load_wblk(p.wblk, nt * 6, lane, W[nt]);
  f32x4 b4[2], sl4[2];   // a lane holds channels 16 nt + 4 kk .. + 3 of ONE position
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) load_bias_slope(p.bias, p.slope, nt, kk, b4[nt], sl4[nt]);
  constexpr int BLOCKS = S2_H / 4;   // 9 row blocks per cube
  const int n_items = p.n_utt * BLOCKS;
  __shared__ int q_next;   // dynamic work items (two workgroups share a CU)
  int item = blockIdx.x;
  while (item < n_items) {
    unsigned q_ticket = 0;
    if (threadIdx.x == 0 && p.queue) q_ticket = atomicAdd(p.queue, 1u);
    const int u = item / BLOCKS, hb = (item - u * BLOCKS) * 4;
    // stage + split: piece e = t + 256 k of thread t = channels 4 (e & 3) .. + 3 of pixel (t >> 2) + 64 k (18 pieces per thread);
    // its four h halves are bytes 8 (piece & 1) .. + 7 of slot `pixel` in plane (piece >> 1), its l halves the same two planes on
    const float* src = p.in + (int64_t)u * (S2_D * S2_H * S2_W * 16);
    {
      int tl = threadIdx.x;
      asm volatile("" : "+v"(tl));   // (keeps this arithmetic inside the item loop)
      const int piece = tl & 3, pix0 = tl >> 2;
      unsigned* const a0s = reg + 4 * ((piece >> 1) * C21H_PIX + pix0) + 2 * (piece & 1);
      const float* const g0 = src + (int64_t)(hb * S2_W + pix0) * 16 + 4 * piece;
      constexpr int PER_D = 4 * S2_W;                    // 72 staged pixels per depth, 648 in the tensor
      constexpr int DSTEP = (S2_H * S2_W - PER_D) * 16;  // floats the source gains per depth on top of 16 pix
      constexpr int NV = 9;
#pragma unroll
      for (int r0 = 0; r0 < 18; r0 += NV) {
        f32x4 sv[NV];
#pragma unroll
        for (int k = r0; k < r0 + NV; ++k) {
          const int d_lo = (64 * k) / PER_D, cross = PER_D * (d_lo + 1) - 64 * k;   // pix0 >= cross: the next depth
          const float* g = g0 + 1024 * k + DSTEP * d_lo;
          if (cross < 64) g = pix0 >= cross ? g + DSTEP : g;
          sv[k - r0] = *reinterpret_cast<const f32x4*>(g);
        }
#pragma unroll
        for (int k = r0; k < r0 + NV; ++k) park_pieces(a0s + 4 * 64 * k, 4 * 2 * C21H_PIX, sv[k - r0], true);
      }
    }
    if (threadIdx.x == 0) q_next = p.queue ? (int)q_ticket + (int)gridDim.x : item + (int)gridDim.x;
    __syncthreads();
    const int item_next = q_next;
    // tiles t = wave + 4 m of 16 positions P = 16 t + i -> (depth P / 56, row (P % 56) / 14, column P % 14); 49 tiles
    static_assert(C21H_POS % 16 == 0 && A2_W == 14, "the position decode below is for 14 columns");
#pragma unroll 1
    for (int t = wave; t < C21H_POS / 16; t += 4) {
      const int P = 16 * t + i;
      const int dq = (P * 1171) >> 16, rem = P - 56 * dq;                       // P / 56 for P < 784
      const int row = (rem * 4682) >> 16, col = rem - 14 * row;                 // rem / 14 for rem < 56
      // input pixel (dq + kd, row, col + kw): slot (dq * 4 + row) * 18 + col + 72 kd + kw of plane (kk & 1) [l: + 2]; tap b = + 1 slot
      const char* const a2 = reinterpret_cast<const char*>(reg) + 16 * ((kk & 1) * C21H_PIX + (dq * 4 + row) * S2_W + col + (kk >= 2 ? 1 : 0));
      auto rd = [&](int pr, int piece) -> u32x4 {
        return *reinterpret_cast<const u32x4*>(a2 + 16 * (72 * (pr >> 1) + 2 * (pr & 1)) + 16 * 2 * C21H_PIX * piece);
      };
      f32x4 acc[2] = {b4[0], b4[1]};
      u32x4 bh[3], bl[3];
      bh[0] = rd(0, 0);
      bl[0] = rd(0, 1);
      bh[1] = rd(1, 0);
      bl[1] = rd(1, 1);
#pragma unroll
      for (int pr = 0; pr < 6; ++pr) {
        if (pr + 2 < 6) {
          bh[(pr + 2) % 3] = rd(pr + 2, 0);
          bl[(pr + 2) % 3] = rd(pr + 2, 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        // (written out, not mfma_pieces: through the helper the prologue's bias and slope loads come out in another order and the
        // kernel measured 1.6 % slower, the two builds alternated three times: 0.2936 - 0.2957 -> 0.2993 - 0.2999 ms per 1 024 cubes)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, W[nt][pr][0]), __builtin_bit_cast(f16x8, bh[pr % 3]), acc[nt], 0, 0, 0);
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, W[nt][pr][0]), __builtin_bit_cast(f16x8, bl[pr % 3]), acc[nt], 0, 0, 0);
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, W[nt][pr][1]), __builtin_bit_cast(f16x8, bh[pr % 3]), acc[nt], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      float* const o = p.out + ((((int64_t)u * A2_D + dq) * S2_H + hb + row) * A2_W + col) * 32 + 4 * kk;
      *reinterpret_cast<f32x4*>(o) = prelu4<SLOPE01>(acc[0], sl4[0]);
      *reinterpret_cast<f32x4*>(o + 16) = prelu4<SLOPE01>(acc[1], sl4[1]);
    }
    __syncthreads();
    item = item_next;
  }
}

// ---- conv2_2 + pool2 through two-piece f16 products: direct form, K = 32 = the 32 input channels of ONE tap, three MFMAs per
// tap (H x h, H x l, L x h), 24 taps.  Item = (cube, pooled column j, third q of the output depths) as before; its input
// [6 d][36 h][2 w][32 c] is split while it is staged: eight planes (four channel quarters x {h, l}) of 16-byte slots, a plane
// split by the parity of the row (rows are 2 apart along a tile): slot ((r & 1) * 6 + d) * 46 + (r >> 1) * 2 + col.  The item's
// 4 d x 15 rows x 2 columns = 120 positions; wave = (N tile nt, plane tile: 16 of a depth's 30 positions) walks the four output depths
// as a depth chain (below): the 48 weight blocks of an N tile are 192 VGPRs.  Pool = max over adjacent lanes (the column pair),
// the even lane stores four channels.
//   in   [n][14][36][14][32]          out  [n][12][15][7][32]
//   wblk [2 nt][24 taps][2][64]: lane (co = 16 nt + (l & 15), kk): e: W[co][8 kk + e][kd][kh], tap = 8 kd + kh ----
// Depth pitch 46, not 36, comes from the tiles of 16 consecutive positions that ran on from one depth's 30 to the next (46 = 30
// (mod 16): their slots mod 16 ran on too); a plane tile's sixteen slots are consecutive at any pitch, and the layout is kept as it was
constexpr int C22H_DP = 46;
constexpr int C22H_PLANE = 560;                      // 2 * 6 * 46 = 552 slots per plane, padded to a multiple of 16
constexpr int C22H_LDS_WORDS = 4 * 8 * C22H_PLANE;   // 71 680 bytes
constexpr int C22H_POS = 4 * O2_H * 2;               // 120 positions per item

template <bool SLOPE01>
__global__ __launch_bounds__(256, 2) void c3d2_conv22h_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem_c22w[];
  unsigned* const reg = reinterpret_cast<unsigned*>(smem_c22w);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, kk = lane >> 4;
  const int nt = wave & 1, half = wave >> 1;
  u32x4 W[24][2];
  load_wblk(p.wblk, nt * 24, lane, W);
  f32x4 b4, sl4;   // channels 16 nt + 4 kk .. + 3 of ONE position
  load_bias_slope(p.bias, p.slope, nt, kk, b4, sl4);
  constexpr int PER_CUBE = O2_W * (O2_D / 4);   // 7 x 3 items
  const int n_items = p.n_utt * PER_CUBE;
  __shared__ int q_next;
  int item = blockIdx.x;
  while (item < n_items) {
    unsigned q_ticket = 0;
    if (threadIdx.x == 0 && p.queue) q_ticket = atomicAdd(p.queue, 1u);
    const int u = item / PER_CUBE, rem = item - u * PER_CUBE, q = rem / O2_W, j = rem - q * O2_W;
    // stage + split: piece e = t + 256 k: channels 4 (e & 7) .. + 3 of pixel (dh = (t >> 4) + 16 k, column (e >> 3) & 1), dh = d * 36 + h
    const float* src = p.in + ((int64_t)u * A2_D + 4 * q) * (S2_H * A2_W * 32) + 2 * j * 32;
    {
      int tl = threadIdx.x;
      asm volatile("" : "+v"(tl));
      const int piece = tl & 7, wq = (tl >> 3) & 1, dh0 = tl >> 4;
      const float* const g0 = src + dh0 * (A2_W * 32) + wq * 32 + 4 * piece;
      constexpr int NV = 7;   // (all 14 in flight spill: the 192 weight registers stay live)
#pragma unroll
      for (int r0 = 0; r0 < 14; r0 += NV) {
        f32x4 sv[NV];
#pragma unroll
        for (int k = r0; k < r0 + NV; ++k)
          if (k < 13 || tl < 128) sv[k - r0] = *reinterpret_cast<const f32x4*>(g0 + (int64_t)(16 * k) * (A2_W * 32));
#pragma unroll
        for (int k = r0; k < r0 + NV; ++k) {
          // dh = dh0 + 16 k -> (d, h): 16 k = 36 d_lo + h_lo at compile time, one comparison for the carry
          const int d_lo = (16 * k) / S2_H, h_lo = 16 * k - S2_H * d_lo;
          int hh = dh0 + h_lo, d = d_lo;
          if (h_lo + 15 >= S2_H) {
            const bool carry = hh >= S2_H;
            hh = carry ? hh - S2_H : hh;
            d = carry ? d + 1 : d;
          }
          const int slot = ((hh & 1) * 6 + d) * C22H_DP + (hh >> 1) * 2 + wq;
          unsigned* const dst = reg + 4 * ((piece >> 1) * C22H_PLANE + slot) + 2 * (piece & 1);
          park_pieces(dst, 4 * 4 * C22H_PLANE, sv[k - r0], k < 13 || tl < 128);
        }
      }
    }
    if (threadIdx.x == 0) q_next = p.queue ? (int)q_ticket + (int)gridDim.x : item + (int)gridDim.x;
    __syncthreads();
    const int item_next = q_next;
    // A DEPTH CHAIN per wave (see c3d2_stage1h_kernel's conv1_2): the kernel is (3, 8, 1), so the fragment of tap (kd, kh) of output
    // (dq, row, col) depends on the input depth dq + kd alone.  Wave = (N tile, plane tile `half`: positions 16 half + i of a
    // depth's 30 = 15 rows x 2 columns; the last two lanes of tile 1 are clamped and store nothing) runs the item's four output
    // depths over its six input depths: the sixteen fragments (kh = 0 .. 7, h and l) of an input depth are read ONCE and
    // multiplied into three live accumulators -- taps 0 - 7 of output dd, 8 - 15 of dd - 1, 16 - 23 of dd - 2.  96 reads per wave
    // where four tiles read 192; every output still receives taps 0 .. 23 in order with the same operands: bit-identical.
    {
      static_assert(C22H_POS == 4 * 2 * O2_H, "four output depths of 15 rows x 2 columns");
      const int r30 = min(16 * half + i, 2 * O2_H - 1), row = r30 >> 1;
      // input pixel (dd, 2 row + kh, col), channels 8 kk .. + 7: slot ((kh & 1) * 6 + dd) * 46 + (row + kh / 2) * 2 + col of plane kk [l: + 4]
      const char* const a2 = reinterpret_cast<const char*>(reg) + 16 * (kk * C22H_PLANE + r30);
      // unit n = 8 s + kh: fragments TWO units ahead (three rotating sets)
      auto rd = [&](int n, int piece) -> u32x4 {
        const int s = n >> 3, kh = n & 7;
        return *reinterpret_cast<const u32x4*>(a2 + 16 * (((kh & 1) * 6 + s) * C22H_DP + (kh >> 1) * 2) + 16 * 4 * C22H_PLANE * piece);
      };
      float* const obase = p.out + ((((int64_t)u * O2_D + 4 * q) * O2_H + row) * O2_W + j) * 32 + 16 * nt + 4 * kk;
      f32x4 acc[4];
      u32x4 bh[3], bl[3];
      bh[0] = rd(0, 0);
      bl[0] = rd(0, 1);
      bh[1] = rd(1, 0);
      bl[1] = rd(1, 1);
#pragma unroll
      for (int n = 0; n < 48; ++n) {
        if (n + 2 < 48) {
          bh[(n + 2) % 3] = rd(n + 2, 0);
          bl[(n + 2) % 3] = rd(n + 2, 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        const int s = n >> 3, kh = n & 7;
#pragma unroll
        for (int kd = 0; kd < 3; ++kd) {
          const int o = s - kd, tap = 8 * kd + kh;
          if (o >= 0 && o < 4) acc[o] = mfma_pieces(W[tap][0], W[tap][1], bh[n % 3], bl[n % 3], tap == 0 ? b4 : acc[o]);
        }
        if (kh == 7 && s >= 2)
          prelu_pool_store<SLOPE01>(acc[s - 2], sl4, obase + (s - 2) * (O2_H * O2_W * 32), (i & 1) == 0 && 16 * half + i < 2 * O2_H);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
    item = item_next;
  }
}

// ---- The second block as ONE kernel: conv2_1 streamed into conv2_2 by depth through LDS.  conv2_1 is (3, 1, 4) -- no extent along
// rows -- and conv2_2 (3, 8, 1) -- none along columns -- so one pooled output column j needs conv2_1's two columns 2 j, 2 j + 1 and
// nothing else, and conv2_2's depth chain consumes them in the order a conv2_1 that walks depth too produces them: the activation
// [14][36][14][32] (2.06 of the pair's 2.9 MB of HBM traffic per cube) only ever exists as two depth pairs in LDS.
// Item = (cube, pooled column j), 7 per cube; one workgroup of eight waves per CU; a STEP is one depth pair of conv2_1's output:
//   * waves 0 - 3 (producers; wave = (N tile, tiles 0 - 4 | 5 - 8)) compute the pair's 2 d x 36 rows x 2 columns = 144 positions = 9
//     full tiles of conv2_1 from four input depths, PReLU, split into (h, l) and park them in the activation ring in conv2_2's
//     plane order (pieces are made where a value is produced: conv2_2's re-split of staged scratch is gone).  They also fetch the
//     input depth pair two steps ahead (columns 2 j .. 2 j + 4 of d_in, 23 KB) at the top of the step and split + park it behind
//     their tiles; at an item's last step, the first two pairs of the next item;
//   * waves 4 - 7 (consumers; wave = (N tile, plane tile), c3d2_conv22h_kernel's wave) multiply the pair of the step BEFORE into
//     their depth chain: two accumulators are carried from step to step (outputs 2 t - 2 with 16 taps, 2 t - 1 with 8), two start.
// One workgroup barrier per step, outside the role branches; 7 steps per item, the steps run on across items (the consumers drain
// an item's last pair while the producers fill the next item's first).  Every output receives its blocks in the order of the two
// kernels above, from the bias, with the same operands: bit-identical to them, per entry point.
//   input ring    [4 planes: h c0-7, h c8-15, l c0-7, l c8-15][8 depth slots: depth & 7][36 rows][5 columns + 1]: pitch 6 makes the
//                 16 slots of a tile (8 rows x 2 columns) distinct mod 16; 110 592 bytes
//   activation    [8 planes: four channel quarters x {h, l}][2 pairs x 2 depths][row parity][18 x 2]; 36 864 bytes
constexpr int S2S_IN_DSLOT = S2_H * 6;                    // 216 slots per input depth
constexpr int S2S_IN_PLANE = 8 * S2S_IN_DSLOT;            // 1 728 slots
constexpr int S2S_IN_WORDS = 4 * 4 * S2S_IN_PLANE;        // 27 648 words
constexpr int S2S_ACT_DSLOT = 2 * S2_H;                   // 72 slots per activation depth
constexpr int S2S_ACT_PLANE = 4 * S2S_ACT_DSLOT;          // 288 slots
constexpr int S2S_ACT_WORDS = 4 * 8 * S2S_ACT_PLANE;      // 9 216 words
constexpr int S2S_LDS_WORDS = S2S_IN_WORDS + S2S_ACT_WORDS;   // 147 456 bytes
constexpr int S2S_STATIC_LDS = 272;                       // q_next (padded to 16) + bs22: the kernel's static LDS, beside the dynamic rings
constexpr int S2S_PIECES = 2 * S2_H * 5 * 4;              // 1 440 sixteen-byte pieces of an input depth pair: [2 d][36 rows][5 w][4]
static_assert(S2S_IN_PLANE % 16 == 0 && S2S_ACT_PLANE % 16 == 0, "the lanes of an LDS lane group sit in different planes");

struct Stage2Params {
  const float* in;      // [n][16][36][18][16]
  const u32x4* w21;     // conv2_1's blocks, as c3d2_conv21h_kernel takes them
  const float *bias21, *slope21;
  const u32x4* w22;     // conv2_2's blocks, as c3d2_conv22h_kernel takes them
  const float *bias22, *slope22;
  float* out;           // [n][12][15][7][32]
  int32_t n_utt;
  unsigned* queue;
};

// A producer lane's step-invariant addresses.  None depends on the data, the item or (but for a ring's depth-slot base, a wave-uniform
// scalar) the step, so they are computed ONCE per kernel (s2s_lane_addr) and only scalars are added inside the step: decoded per
// tile and per piece they were 25 of a tile's 37 vector instructions and 24 in front of a fetch's six loads, on the SIMD whose matrix
// pipe the same waves feed.  Byte offsets; the compiler is kept from rematerialising the arithmetic where they are used
// (s2s_lane_addr's empty asm statements).
struct S2sLane {
  // the wave's four REGULAR tiles 5 half + k, k = 0 .. 3: position 16 (5 half + k) + i = (dd = half, row = 4 half + 8 k + (i >> 1),
  // col = i & 1).  in_reg, act_reg: tile k = 0 in the input ring (depth slot 0) and in the activation ring (depth slot half); tile
  // k is S2S_TILE_IN / S2S_TILE_ACT bytes on
  unsigned in_reg, act_reg;
  // tile 4 (the waves of half 0 only): lanes i < 8 = (dd 0, rows 32 - 35), lanes i >= 8 = (dd 1, rows 0 - 3)
  unsigned in_t4, act_t4;
  // piece e = tp + 256 m of producer thread tp: channels 4 (e & 3) .. + 3 of pixel (dd = q / 36, row q % 36, column (e % 20) / 4),
  // q = e / 20: its bytes from the depth pair's first float at column 2 j, and its h words from the pair's first depth slot
  unsigned fetch[6], park[6];
};
constexpr int S2S_TILE_IN = 16 * 8 * 6, S2S_TILE_ACT = 16 * 8;   // eight rows on: 48 slots of the input ring, 8 of the activation ring
// conv2_1 position (row, col), lane group kk: plane (kk & 1) [l: + 2] of the input ring; tap b = + 1 slot
__device__ __forceinline__ unsigned s2s_in_off(int kk, int row, int col) {
  return 16 * ((kk & 1) * S2S_IN_PLANE + row * 6 + col + (kk >= 2 ? 1 : 0));
}
// channels 16 nt + 4 kk .. + 3 of position (dd, row, col): plane 2 nt + kk / 2 [l: + 4], bytes 8 (kk & 1) .. + 7 of its slot
__device__ __forceinline__ unsigned s2s_act_off(int nt, int kk, int dd, int row, int col) {
  const int slot = dd * S2S_ACT_DSLOT + (row & 1) * S2_H + (row >> 1) * 2 + col;
  return 4 * (4 * ((2 * nt + (kk >> 1)) * S2S_ACT_PLANE + slot) + 2 * (kk & 1));
}
__device__ __forceinline__ S2sLane s2s_lane_addr(int lane, int nt, int half, int tp) {
  const int i = lane & 15, kk = lane >> 4, col = i & 1;
  S2sLane A;
  A.in_reg = s2s_in_off(kk, 4 * half + (i >> 1), col);
  A.act_reg = s2s_act_off(nt, kk, half, 4 * half + (i >> 1), col);
  A.in_t4 = s2s_in_off(kk, i < 8 ? 32 + (i >> 1) : (i - 8) >> 1, col);
  A.act_t4 = s2s_act_off(nt, kk, i < 8 ? 0 : 1, i < 8 ? 32 + (i >> 1) : (i - 8) >> 1, col);
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    // (threads past the last piece load it again and park nothing: a load under a condition of its own made the compiler wait
    // for every load of the pair right behind their issue)
    const int ef = min(tp + 256 * m, S2S_PIECES - 1), qf = (ef * 3277) >> 16, rf = ef - 20 * qf;   // e / 20 for e < 1 536
    A.fetch[m] = 4 * (qf * (S2_W * 16) + 4 * rf);
    const int e = tp + 256 * m, q = (e * 3277) >> 16, r = e - 20 * q;
    const int dd = q >= S2_H ? 1 : 0, row = q - S2_H * dd, c = r >> 2, piece = r & 3;
    A.park[m] = 4 * (4 * ((piece >> 1) * S2S_IN_PLANE + dd * S2S_IN_DSLOT + row * 6 + c) + 2 * (piece & 1));
  }
  asm volatile("" : "+v"(A.in_reg), "+v"(A.act_reg), "+v"(A.in_t4), "+v"(A.act_t4));
#pragma unroll
  for (int m = 0; m < 6; ++m) asm volatile("" : "+v"(A.fetch[m]), "+v"(A.park[m]));
  return A;
}

// input depths D0, D0 + 1 of the item whose column 2 j starts at col0: one wave-uniform base + the lane's six offsets, as loads with a
// scalar base and a 32-bit offset register.  (The offsets pass through an empty asm statement HERE, in place: the compiler otherwise
// widens them to 64 bits once, outside the step loop, and adds the base to each pair with a 64-bit vector add per piece.)
__device__ __forceinline__ void s2s_fetch(const float* col0, int D0, S2sLane& A, f32x4 (&sv)[6]) {
  const char* const base = reinterpret_cast<const char*>(col0 + D0 * (S2_H * S2_W * 16));
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    asm volatile("" : "+v"(A.fetch[m]));
    sv[m] = *reinterpret_cast<const f32x4*>(base + A.fetch[m]);
  }
}
// (D0 is even: depth D0 + dd lies in depth slot (D0 & 7) + dd)
__device__ __forceinline__ void s2s_park(unsigned* in_lds, int D0, int tp, const S2sLane& A, const f32x4 (&sv)[6]) {
  char* const base = reinterpret_cast<char*>(in_lds + 4 * (D0 & 7) * S2S_IN_DSLOT);
#pragma unroll
  for (int m = 0; m < 6; ++m)
    park_pieces(reinterpret_cast<unsigned*>(base + A.park[m]), 4 * 2 * S2S_IN_PLANE, sv[m], tp + 256 * m < S2S_PIECES);
}

// One tile of conv2_1: 16 positions; a2[kd] = the lane's fragment of input depth kd of the tile's three (h plane, tap a), dst = its
// four channels' h words in the activation ring
template <bool SLOPE01>
__device__ __forceinline__ void s2s_conv21_tile(const char* const (&a2)[3], unsigned* dst, const u32x4 (&W)[6][2], f32x4 b4, f32x4 sl4) {
  // (fragments fetched across tiles -- pairs 4 and 5 of a tile reading pairs 0 and 1 of the next -- measured 3 - 4 % SLOWER)
  auto rd = [&](int pr, int piece) -> u32x4 {
    return *reinterpret_cast<const u32x4*>(a2[pr >> 1] + 16 * 2 * (pr & 1) + 16 * 2 * S2S_IN_PLANE * piece);
  };
  f32x4 acc = b4;
  u32x4 bh[3], bl[3];
  bh[0] = rd(0, 0);
  bl[0] = rd(0, 1);
  bh[1] = rd(1, 0);
  bl[1] = rd(1, 1);
#pragma unroll
  for (int pr = 0; pr < 6; ++pr) {
    if (pr + 2 < 6) {
      bh[(pr + 2) % 3] = rd(pr + 2, 0);
      bl[(pr + 2) % 3] = rd(pr + 2, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    acc = mfma_pieces(W[pr][0], W[pr][1], bh[pr % 3], bl[pr % 3], acc);
    __builtin_amdgcn_sched_barrier(0);
  }
  park_pieces(dst, 4 * 4 * S2S_ACT_PLANE, prelu4<SLOPE01>(acc, sl4), true);
}

// conv2_1's output depths 2 t, 2 t + 1 of the item's two columns: the wave's tiles (half 0: tiles 0 - 4, half 1: tiles 5 - 8) of its N
// tile -> activation depth slots act_d0, act_d0 + 1.  Position P = 16 tile + i -> (dd = P / 72, row = (P % 72) / 2, column P % 2); input
// pixel (2 t + dd + kd, row, col + kw) is in depth slot (2 t + dd + kd) & 7.  The step adds wave-uniform scalars to the lane's
// addresses of S2sLane: the depth-slot bases once per step, the tiles at compile-time offsets from them
template <bool SLOPE01>
__device__ __forceinline__ void s2s_conv21_step(const unsigned* in_lds, unsigned* act_lds, int t, int act_d0, int half, bool hi4, const S2sLane& A,
                                                const u32x4 (&W)[6][2], f32x4 b4, f32x4 sl4) {
  const char* const in_b = reinterpret_cast<const char*>(in_lds);
  char* const act_b = reinterpret_cast<char*>(act_lds) + 16 * S2S_ACT_DSLOT * act_d0;
  auto dslot = [&](int d) -> unsigned { return 16 * S2S_IN_DSLOT * ((2 * t + d) & 7); };
  {
    const char* a0[3];
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) a0[kd] = in_b + (A.in_reg + dslot(half + kd));
    char* const d0 = act_b + A.act_reg;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const char* const a2[3] = {a0[0] + S2S_TILE_IN * k, a0[1] + S2S_TILE_IN * k, a0[2] + S2S_TILE_IN * k};
      s2s_conv21_tile<SLOPE01>(a2, reinterpret_cast<unsigned*>(d0 + S2S_TILE_ACT * k), W, b4, sl4);
    }
  }
  if (half == 0) {   // tile 4: the depth of lanes i >= 8 (hi4) is one on
    const char* a2[3];
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) a2[kd] = in_b + (A.in_t4 + (hi4 ? dslot(kd + 1) : dslot(kd)));
    s2s_conv21_tile<SLOPE01>(a2, reinterpret_cast<unsigned*>(act_b + A.act_t4), W, b4, sl4);
  }
}

// conv2_2's chain over the activation depths s = 2 tc, 2 tc + 1 at a2 (the lane's slot of depth 2 tc, h plane): accumulators P (output
// 2 tc - 2, taps 0 - 15 done) and Q (2 tc - 1, taps 0 - 7 done) come in and go out one pair on.  KIND 0: tc = 0 (no outputs - 2, - 1),
// 2: tc = 6 (no outputs 12, 13), 1: the rest.  `o2` = the lane's output address at depth 2 tc; bs[0], bs[4] = the lane's bias and slope in
// LDS, read where they are used: beside the 192 weight registers, eight more held across the steps were sixteen spilled
template <bool SLOPE01, int KIND>
__device__ __forceinline__ void s2s_conv22_step(const char* a2, const u32x4 (&W)[24][2], const f32x4* bs, f32x4& P, f32x4& Q, float* o2,
                                                bool store) {
  auto rd = [&](int n, int piece) -> u32x4 {
    const int dd = n >> 3, kh = n & 7;
    return *reinterpret_cast<const u32x4*>(a2 + 16 * (dd * S2S_ACT_DSLOT + (kh & 1) * S2_H + (kh >> 1) * 2) + 16 * 4 * S2S_ACT_PLANE * piece);
  };
  constexpr int OD_STRIDE = O2_H * O2_W * 32;
  f32x4 A = P, B = Q, C = bs[0], D = C, sl4;
  u32x4 bh[3], bl[3];   // fragments two units ahead (three rotating sets), as in c3d2_conv22h_kernel
  bh[0] = rd(0, 0);
  bl[0] = rd(0, 1);
  bh[1] = rd(1, 0);
  bl[1] = rd(1, 1);
#pragma unroll
  for (int n = 0; n < 16; ++n) {
    if (n + 2 < 16) {
      bh[(n + 2) % 3] = rd(n + 2, 0);
      bl[(n + 2) % 3] = rd(n + 2, 1);
    }
    if (KIND != 2 && n == 6) D = bs[0];
    if (KIND != 0 && n == 5) sl4 = bs[4];
    __builtin_amdgcn_sched_barrier(0);
    const int dd = n >> 3, kh = n & 7;
    if (dd == 0) {
      if (KIND != 2) C = mfma_pieces(W[kh][0], W[kh][1], bh[n % 3], bl[n % 3], C);
      if (KIND != 0) B = mfma_pieces(W[8 + kh][0], W[8 + kh][1], bh[n % 3], bl[n % 3], B);
      if (KIND != 0) A = mfma_pieces(W[16 + kh][0], W[16 + kh][1], bh[n % 3], bl[n % 3], A);
      if (KIND != 0 && kh == 7) prelu_pool_store<SLOPE01>(A, sl4, o2 - 2 * OD_STRIDE, store);
    } else {
      if (KIND != 2) D = mfma_pieces(W[kh][0], W[kh][1], bh[n % 3], bl[n % 3], D);
      if (KIND != 2) C = mfma_pieces(W[8 + kh][0], W[8 + kh][1], bh[n % 3], bl[n % 3], C);
      if (KIND != 0) B = mfma_pieces(W[16 + kh][0], W[16 + kh][1], bh[n % 3], bl[n % 3], B);
      if (KIND != 0 && kh == 7) prelu_pool_store<SLOPE01>(B, sl4, o2 - OD_STRIDE, store);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  P = C;
  Q = D;
}

// COMPILER-DEPENDENT (ROCm 7.2's hipcc), this barrier and the two __builtin_amdgcn_s_waitcnt(0x0F70) below: they buy about 10 % of the
// kernel through where the compiler places its waits, not through anything the hardware needs.  After a compiler upgrade rerun
// -Rpass-analysis=kernel-resource-usage (256 VGPRs, no spill, no scratch in both instances), look for `s_waitcnt vmcnt` between the
// producers' global_load_dwordx4 and their first v_mfma in the assembly (there must be none), and time
// `tools/time_network.py 16384 stage2` against SVK_C3D2_STAGE2_TWO_KERNELS=1 (9.20 against 10.21 ms when this was written).
// The step barrier: the LDS traffic of the wave is waited for, its global traffic is not -- __syncthreads() waits for vmcnt(0) as well,
// which here is the consumers' output stores of the step just ended (nothing in the kernel reads them) once per step.
__device__ __forceinline__ void s2s_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// One role's walk over the workgroup's items and steps.  The two roles run the SAME skeleton -- the items in the same order from
// q_next, seven steps per item, one barrier per step and one drain step -- as two instances, so every wave executes the same number
// of barriers; one loop with the roles as branches inside it kept conv2_2's 192 weight registers live on the producers' path as well
// (200 registers spilled).
template <bool SLOPE01, bool PRODUCER>
__device__ __forceinline__ void s2s_run(const Stage2Params& p, unsigned* in_lds, unsigned* act_lds, int* q_next, f32x4* bs22, int lane, int wave) {
  const int i = lane & 15, kk = lane >> 4;
  const int nt = wave & 1, half = (wave >> 1) & 1;
  constexpr int NW = PRODUCER ? 6 : 24;
  u32x4 W[NW][2];
  load_wblk(PRODUCER ? p.w21 : p.w22, nt * NW, lane, W);
  const f32x4* const bs = bs22 + 8 * nt + kk;   // the consumers' bias and slope: [2 nt][bias | slope][4 kk] in LDS
  f32x4 b4, sl4;   // channels 16 nt + 4 kk .. + 3 of ONE position, of the role's layer
  {
    f32x4 b, sl;
    load_bias_slope(PRODUCER ? p.bias21 : p.bias22, PRODUCER ? p.slope21 : p.slope22, nt, kk, b, sl);
    if constexpr (PRODUCER) {
      b4 = b;
      sl4 = sl;
    } else if (i == 0) {   // (both waves of an N tile write the same values)
      bs22[8 * nt + kk] = b;
      bs22[8 * nt + 4 + kk] = sl;
    }
  }
  const int n_items = p.n_utt * O2_W;
  auto col0_of = [&](int it) -> const float* {
    const int u = it / O2_W, j = it - u * O2_W;
    return p.in + (int64_t)u * (S2_D * S2_H * S2_W * 16) + 2 * j * 16;
  };
  int item = blockIdx.x, prev = n_items, nxt = n_items;   // the producers' item, the one before it, the one after it
  const int tp = threadIdx.x & 255;
  S2sLane A;
  if constexpr (PRODUCER) {   // the first item's first two input depth pairs
    A = s2s_lane_addr(lane, nt, half, tp);
    f32x4 sa[6], sb[6];
    s2s_fetch(col0_of(item), 0, A, sa);
    s2s_fetch(col0_of(item), 2, A, sb);
    s2s_park(in_lds, 0, tp, A, sa);
    s2s_park(in_lds, 2, tp, A, sb);
  }
  __syncthreads();
  // every load of the prologue has landed, and the compiler is told so (vmcnt(0) as an instruction it tracks): it keeps no count of
  // loads across the loop's back edge, and with the weights' loads still open in its books it drained the step's input fetch in front
  // of the step's first MFMA
  __builtin_amdgcn_s_waitcnt(0x0F70);
  const int r30 = min(16 * half + i, 2 * O2_H - 1), lane_out = (r30 >> 1) * (O2_W * 32) + 16 * nt + 4 * kk;
  const bool store = (i & 1) == 0 && 16 * half + i < 2 * O2_H;
  f32x4 accP = {0.f, 0.f, 0.f, 0.f}, accQ = accP;   // (the consumers' first step is of KIND 0: it reads neither)
  unsigned q_ticket = 0;
  int gp = 0;   // the activation pair slot the producers fill in this step; the consumers read the other one
  for (;;) {
#pragma unroll 1
    for (int t = 0; t < 7; ++t) {
      const bool live = item < n_items;
      if constexpr (PRODUCER) {
        // (nothing is in flight at a step's top -- every fetch was parked -- but the compiler's books carry the previous step's loads
        // across the back edge and it waits for them again in the middle of this step's fetch: vmcnt(0) here, a no-op, clears them)
        __builtin_amdgcn_s_waitcnt(0x0F70);
        // (the ticket is drawn a step before it is needed: its round trip hides behind that step's tiles)
        if (t == 4 && threadIdx.x == 0 && p.queue) q_ticket = atomicAdd(p.queue, 1u);
        if (live) {
          // input depth pair t + 2 of the item; at its last step pairs 0 and 1 of the next item (their depth slots 0 .. 3 were last read
          // in step 5)
          const int fitem = t < 6 ? item : nxt, fD = t < 6 ? 2 * t + 4 : 0;
          const bool fa = fitem < n_items, fb = fa && t == 6;
          f32x4 sa[6], sb[6];
          if (fa) s2s_fetch(col0_of(fitem), fD, A, sa);
          if (fb) s2s_fetch(col0_of(fitem), 2, A, sb);
          s2s_conv21_step<SLOPE01>(in_lds, act_lds, t, 2 * gp, half, i >= 8, A, W, b4, sl4);
          if (fa) s2s_park(in_lds, fD, tp, A, sa);
          if (fb) s2s_park(in_lds, 2, tp, A, sb);
        }
        if (t == 5 && threadIdx.x == 0) *q_next = p.queue ? (int)q_ticket + (int)gridDim.x : item + (int)gridDim.x;
      } else {
        const int ci = t == 0 ? prev : item, tc = t == 0 ? 6 : t - 1;   // the pair of the step before
        if (ci < n_items) {
          const int u = ci / O2_W, j = ci - u * O2_W;
          const char* const a2 = reinterpret_cast<const char*>(act_lds) + 16 * (kk * S2S_ACT_PLANE + 2 * (gp ^ 1) * S2S_ACT_DSLOT + r30);
          float* const o2 = p.out + (((int64_t)u * O2_D + 2 * tc) * (O2_H * O2_W) + j) * 32 + lane_out;   // (a scalar base + one register)
          if (tc == 0) s2s_conv22_step<SLOPE01, 0>(a2, W, bs, accP, accQ, o2, store);
          else if (tc == 6) s2s_conv22_step<SLOPE01, 2>(a2, W, bs, accP, accQ, o2, store);
          else s2s_conv22_step<SLOPE01, 1>(a2, W, bs, accP, accQ, o2, store);
        }
      }
      s2s_barrier();
      gp ^= 1;
      if (t == 0 && !live) return;   // the last item's last pair is consumed
      if (t == 5) nxt = __builtin_amdgcn_readfirstlane(*q_next);
    }
    prev = item;
    item = nxt;
  }
}

template <bool SLOPE01>
__global__ __launch_bounds__(512) void c3d2_stage2h_kernel(const Stage2Params p) {
  extern __shared__ __attribute__((aligned(16))) float smem_s2s[];
  unsigned* const in_lds = reinterpret_cast<unsigned*>(smem_s2s);
  unsigned* const act_lds = in_lds + S2S_IN_WORDS;
  __shared__ int q_next;
  __shared__ f32x4 bs22[16];
  static_assert(sizeof(bs22) + 16 == S2S_STATIC_LDS, "S2S_STATIC_LDS states this kernel's static LDS");
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave < 4) s2s_run<SLOPE01, true>(p, in_lds, act_lds, &q_next, bs22, lane, wave);
  else s2s_run<SLOPE01, false>(p, in_lds, act_lds, &q_next, bs22, lane, wave);
}

// ---- conv3_1 (32 -> 64, kernel (3,1,3)) + BN + PReLU (model.py:126-128, :159-161) through two-piece f16 products: direct
// form, K = 32 = the 32 input channels of ONE tap, three MFMAs per tap, 9 taps.  No taps along h, so item = (cube, block of 3
// rows): region 12 depths x 3 rows x 7 columns of 32 channels, split into (h, l) while staged: eight planes (four channel quarters
// x {h, l}) of 16-byte slots, slot = pixel (d * 3 + row) * 7 + col (32 KB; three workgroups per CU).  The item's 10 d x 3 rows x
// 5 columns = 150 positions are 9.4 tiles of 16 consecutive positions; wave = N tile (16 of the 64 output channels: 18 weight
// blocks = 72 VGPRs), every wave walks all ten tiles.  Output chunked and column-major, 16-byte stores.
//   in   [n][12][15][7][32]           out  [n][10][8 chunks][5 w][15 h][8] (what svk_c3d2_conv32t stages)
//   wblk [4 nt][9 taps][2][64]: lane (co = 16 nt + (l & 15), kk): e: W[co][8 kk + e][kd][kw], tap = 3 kd + kw ----
constexpr int C31H_PLANE = 256;                               // 12 * 3 * 7 = 252 slots per plane, padded to a multiple of 16: the lanes of an LDS
                                                              // lane group sit in different planes (kk) and must not land on each other's slots
constexpr int C31H_LDS_WORDS = 4 * 8 * C31H_PLANE;            // 32 768 bytes
constexpr int C31H_POS = 10 * 3 * 5;                          // 150 positions per item

template <bool SLOPE01>
__global__ __launch_bounds__(256, 3) void c3d2_conv31h_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem_c31[];
  unsigned* const reg = reinterpret_cast<unsigned*>(smem_c31);
  const int lane = threadIdx.x & 63, nt = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, kk = lane >> 4;
  u32x4 W[9][2];
  load_wblk(p.wblk, nt * 9, lane, W);
  f32x4 b4, sl4;   // channels 16 nt + 4 kk .. + 3 of ONE position
  load_bias_slope(p.bias, p.slope, nt, kk, b4, sl4);
  const int n_items = p.n_utt * 5;
  __shared__ int q_next;   // dynamic work items: see c3d2_conv21h_kernel (three workgroups share a CU here)
  int item = blockIdx.x;
  while (item < n_items) {
    unsigned q_ticket = 0;
    if (threadIdx.x == 0 && p.queue) q_ticket = atomicAdd(p.queue, 1u);
    const int u = item / 5, rb = item - u * 5;
    // stage + split [12 d][3 rows][7 w][32 c]: per depth 672 contiguous floats = 168 sixteen-byte pieces; 2 016 in all, eight per
    // thread.  piece e = t + 256 k = channels 4 (e & 7) .. + 3 of pixel e >> 3 (168 d is a multiple of 8: the pixel index has no d
    // in it and is linear in k); the source is 4 e + 2 688 d floats, and for a compile-time k the depth d = e / 168 is a constant
    // plus at most two comparisons of t with the window's boundaries
    const float* src = p.in + ((int64_t)u * 12 * 15 + 3 * rb) * (7 * 32);
    {
      int tl = threadIdx.x;
      asm volatile("" : "+v"(tl));   // (keeps this arithmetic inside the item loop)
      const int c4 = tl & 7;
      unsigned* const a0s = reg + 4 * ((c4 >> 1) * C31H_PLANE + (tl >> 3)) + 2 * (c4 & 1);
      const float* const g0 = src + 4 * tl;
      constexpr int DSTEP = 15 * 7 * 32 - 4 * 168;   // floats the source gains per depth on top of 4 e
      f32x4 sv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int d_lo = (256 * k) / 168, c1 = 168 * (d_lo + 1) - 256 * k, c2 = c1 + 168;   // t >= c1 (c2): one (two) depths on
        const float* g = g0 + 1024 * k + DSTEP * d_lo;
        if (c1 < 256) g = tl >= c1 ? g + DSTEP : g;
        if (c2 < 256) g = tl >= c2 ? g + DSTEP : g;
        if (256 * k + 255 < 2016 || tl < 2016 - 256 * k) sv[k] = *reinterpret_cast<const f32x4*>(g);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) park_pieces(a0s + 4 * 32 * k, 4 * 4 * C31H_PLANE, sv[k], 256 * k + 255 < 2016 || tl < 2016 - 256 * k);
    }
    if (threadIdx.x == 0) q_next = p.queue ? (int)q_ticket + (int)gridDim.x : item + (int)gridDim.x;
    __syncthreads();
    const int item_next = q_next;
#pragma unroll 1
    for (int t = 0; t < (C31H_POS + 15) / 16; ++t) {
      const int P = min(16 * t + i, C31H_POS - 1);
      const int dq = (P * 4370) >> 16, r15 = P - 15 * dq;                       // P / 15 for P < 150
      const int row = (r15 * 13108) >> 16, col = r15 - 5 * row;                 // r15 / 5 for r15 < 15
      // input pixel (dq + kd, row, col + kw), channels 8 kk .. + 7: slot (dq * 3 + row) * 7 + col + 21 kd + kw of plane kk [l: + 4]
      const char* const a2 = reinterpret_cast<const char*>(reg) + 16 * (kk * C31H_PLANE + (dq * 3 + row) * 7 + col);
      auto rd = [&](int tap, int piece) -> u32x4 {
        return *reinterpret_cast<const u32x4*>(a2 + 16 * (21 * (tap / 3) + tap % 3) + 16 * 4 * C31H_PLANE * piece);
      };
      f32x4 acc = b4;
      u32x4 bh[3], bl[3];
      bh[0] = rd(0, 0);
      bl[0] = rd(0, 1);
      bh[1] = rd(1, 0);
      bl[1] = rd(1, 1);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        if (tap + 2 < 9) {
          bh[(tap + 2) % 3] = rd(tap + 2, 0);
          bl[(tap + 2) % 3] = rd(tap + 2, 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        acc = mfma_pieces(W[tap][0], W[tap][1], bh[tap % 3], bl[tap % 3], acc);
        __builtin_amdgcn_sched_barrier(0);
      }
      // chunked, column-major output [d][chunk = 2 nt + (kk >> 1)][w][h][8]: the lane's four channels are 16 contiguous bytes
      if (16 * t + i < C31H_POS) {
        float* const o = p.out + ((((int64_t)u * 10 + dq) * 8 + 2 * nt + (kk >> 1)) * 5 + col) * (15 * 8) + (3 * rb + row) * 8 + 4 * (kk & 1);
        *reinterpret_cast<f32x4*>(o) = prelu4<SLOPE01>(acc, sl4);
      }
    }
    __syncthreads();
    item = item_next;
  }
}

// ---- conv3_2 (64 -> 64, kernel (3,7,1)) + BN + PReLU (model.py:129-131, :162-164) through two-piece f16 products, direct form:
// 21 taps x two K = 32 blocks (channels 0-31 | 32-63) x three MFMAs.  No taps along w, and conv3_1 writes its output chunked and
// COLUMN-major, so item = (cube, column): 10 d x 15 h x 64 c = eighty 480-byte runs, split into (h, l) while staged: sixteen planes
// (eight channel chunks x {h, l}) of 16-byte slots, slot = d * 15 + h (38 KB).  Outputs 8 d x 9 h = 72 positions = 4.5 tiles.  The
// weight blocks of an N tile and ONE K block are 168 VGPRs: wave = (N tile nt, K block kb), eight waves; the two waves of an N tile
// swap partial sums through LDS (kb 0 finishes tiles 0 - 2, kb 1 tiles 3 - 4).  The next item's runs are loaded into registers in
// front of the tiles and parked behind them: one workgroup per CU, its memory latency under its own matrix work.
// (As an instance of c3d2_tail.hip's f32 batch-GEMM kernel when that was a template, Winograd F(2,3) along depth: 1.34 - 1.62 ms per 4 018 cubes.)
//   in   [n][10][8 chunks][5 w][15 h][8]          out  [n][8 d][8 chunks][45 = 9 h x 5 w][8]
//   wblk [4 nt][2 kb][21 taps][2][64]: lane (co = 16 nt + (l & 15), kk): e: W[co][32 kb + 8 kk + e][kd][kh], tap = 7 kd + kh ----
// depth pitch 25, not 15: a tile's positions run on from one depth's 9 rows to the next, and with 25 = 9 (mod 16) so do their slots
// mod 16 (see C22H_DP)
constexpr int C32H_DP = 25;
constexpr int C32H_PLANE = 256;                               // 10 * 25 = 250 slots per plane, padded to a multiple of 16 (see C31H_PLANE)
constexpr int C32H_LDS_WORDS = 4 * 16 * C32H_PLANE;           // 65 536 bytes
constexpr int C32H_XCH_FLOATS = 8 * 5 * 64 * 4;               // [wave = nt + 4 kb][tile][lane] f32x4: every wave's partial sums
constexpr int C32H_POS = 8 * 9;                               // 72 positions per item

template <bool SLOPE01>
__global__ __launch_bounds__(512) void c3d2_conv32h_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem_c32[];
  unsigned* const reg = reinterpret_cast<unsigned*>(smem_c32);
  float* const xch = smem_c32 + C32H_LDS_WORDS;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, kk = lane >> 4;
  const int nt = wave & 3, kb = wave >> 2;
  u32x4 W[21][2];
  load_wblk(p.wblk, (nt * 2 + kb) * 21, lane, W);
  f32x4 b4, sl4;   // channels 16 nt + 4 kk .. + 3 of ONE position (the bias rides in K block 0's accumulators)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    b4[r] = kb == 0 ? p.bias[16 * nt + 4 * kk + r] : 0.f;
    sl4[r] = p.slope[16 * nt + 4 * kk + r];
  }
  const int n_items = p.n_utt * 5;
  __shared__ int q_next;
  // piece e = t + 512 k (five per thread, 2 400 in all): run e / 30 = d * 8 + chunk, h = (e % 30) / 2, channels 4 (e & 1) .. + 3 of the chunk
  f32x4 sv[5];
  auto load_item = [&](int it) {
    const int u = it / 5, w = it - 5 * u;
    const float* const src = p.in + (int64_t)u * (10 * 8 * 5 * 120) + w * 120;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int e = (int)threadIdx.x + 512 * k;
      const int run = (e * 2185) >> 16, r = e - 30 * run;       // e / 30 for e < 2 400
      if (k < 4 || threadIdx.x < 2400 - 4 * 512) sv[k] = *reinterpret_cast<const f32x4*>(src + run * 600 + 4 * r);
    }
  };
  auto park_item = [&]() {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int e = (int)threadIdx.x + 512 * k;
      const int run = (e * 2185) >> 16, r = e - 30 * run;
      const int d = run >> 3, chunk = run & 7;
      unsigned* const dst = reg + 4 * (chunk * C32H_PLANE + d * C32H_DP + (r >> 1)) + 2 * (r & 1);
      park_pieces(dst, 4 * 8 * C32H_PLANE, sv[k], k < 4 || threadIdx.x < 2400 - 4 * 512);
    }
  };
  // items: the first two of a workgroup at a fixed stride, every later one drawn from the device-wide counter ONE item ahead (the
  // next item's runs are fetched during this item; its ticket's round trip runs under this item's tiles)
  int item = blockIdx.x, item_next = item + (int)gridDim.x;
  if (item < n_items) {
    load_item(item);
    park_item();
  }
  __syncthreads();
  while (item < n_items) {
    unsigned q_ticket = 0;
    if (threadIdx.x == 0 && p.queue) q_ticket = atomicAdd(p.queue, 1u);
    const int u = item / 5, w = item - 5 * u;
    if (item_next < n_items) load_item(item_next);
#pragma unroll 1
    for (int t = 0; t < 5; ++t) {
      const int P = min(16 * t + i, C32H_POS - 1);
      const int dq = (P * 7282) >> 16, row = P - 9 * dq;                        // P / 9 for P < 72
      // input pixel (dq + kd, row + kh), channels 32 kb + 8 kk .. + 7: slot (dq + kd) * 25 + row + kh of plane 4 kb + kk [l: + 8]
      const char* const a2 = reinterpret_cast<const char*>(reg) + 16 * ((4 * kb + kk) * C32H_PLANE + dq * C32H_DP + row);
      auto rd = [&](int tap, int piece) -> u32x4 {
        return *reinterpret_cast<const u32x4*>(a2 + 16 * (C32H_DP * (tap / 7) + tap % 7) + 16 * 8 * C32H_PLANE * piece);
      };
      f32x4 a = b4;
      u32x4 bh[2], bl[2];   // (one tap ahead: a second set ahead is eight registers more)
      bh[0] = rd(0, 0);
      bl[0] = rd(0, 1);
#pragma unroll
      for (int tap = 0; tap < 21; ++tap) {
        if (tap + 1 < 21) {
          bh[(tap + 1) & 1] = rd(tap + 1, 0);
          bl[(tap + 1) & 1] = rd(tap + 1, 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        a = mfma_pieces(W[tap][0], W[tap][1], bh[tap & 1], bl[tap & 1], a);
        __builtin_amdgcn_sched_barrier(0);
      }
      // partial sums over this wave's K block -> LDS (kept in registers for the tiles a wave finishes they cost 12 VGPRs this kernel
      // does not have: the 168 weight registers and the 20 of the next item's runs leave room for one accumulator)
      *reinterpret_cast<f32x4*>(xch + ((wave * 5 + t) * 64 + lane) * 4) = a;
    }
    __syncthreads();   // both K blocks' partial sums are in LDS; nobody reads the planes any more
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const bool mine = kb == 0 ? t < 3 : t >= 3;   // wave-uniform: K block 0's wave finishes tiles 0 - 2, K block 1's tiles 3 - 4
      if (mine) {
        const int P = 16 * t + i;
        const int Pc = min(P, C32H_POS - 1);
        const int dq = (Pc * 7282) >> 16, row = Pc - 9 * dq;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xch + ((nt * 5 + t) * 64 + lane) * 4) +
                        *reinterpret_cast<const f32x4*>(xch + (((nt + 4) * 5 + t) * 64 + lane) * 4);
        if (P < C32H_POS) {
          float* const o = p.out + ((((int64_t)u * 8 + dq) * 8 + 2 * nt + (kk >> 1)) * 45 + row * 5 + w) * 8 + 4 * (kk & 1);
          *reinterpret_cast<f32x4*>(o) = prelu4<SLOPE01>(v, sl4);
        }
      }
    }
    if (item_next < n_items) park_item();
    if (threadIdx.x == 0) q_next = p.queue ? (int)q_ticket + 2 * (int)gridDim.x : item_next + (int)gridDim.x;
    __syncthreads();   // the next item's planes are written; the exchange buffer is free
    item = item_next;
    item_next = q_next;
  }
}

// ---- conv4_1 (64 -> 128, kernel (3,1,3)) + BN + PReLU (model.py:132-135, :165-166) through two-piece f16 products, direct form:
// 9 taps x two K = 32 blocks x three MFMAs.  Item = ONE CUBE: its whole input [8 d][8 chunks][45 = 9 h x 5 w][8] (92 KB) is split
// while staged into sixteen planes (eight channel chunks x {h, l}) of 16-byte slots, slot = d * 59 + 9 w + h; outputs 6 d x 9 h x 3 w =
// 162 positions = 10.1 tiles; wave = N tile (eight waves: 128 output channels; 36 weight blocks = 144 VGPRs), every wave walks all
// eleven tiles.  The next cube is loaded into registers in front of the tiles and parked behind them.
// (As an instance of c3d2_tail.hip's f32 batch-GEMM kernel when that was a template, Winograd F(2,3) along depth: 0.54 - 0.69 ms per 4 018 cubes.)
//   in   [n][8][8 chunks][45][8]                  out  [n][6 d][16 chunks][27 = 9 h x 3 w][8]
//   wblk [8 nt][9 taps][2 kb][2][64]: lane (co = 16 nt + (l & 15), kk): e: W[co][32 kb + 8 kk + e][kd][kw], tap = 3 kd + kw ----
// A plane holds [8 d][5 w][9 h] at depth pitch 59: positions are walked (depth, column, row) with the row fastest, 27 per depth, and
// 59 = 27 (mod 16), so sixteen consecutive positions are sixteen consecutive slots mod 16 at every tap (see C22H_DP)
constexpr int C41H_DP = 59;
constexpr int C41H_PLANE = 480;                               // 8 * 59 = 472 slots per plane, padded to a multiple of 16
constexpr int C41H_LDS_WORDS = 4 * 16 * C41H_PLANE;           // 122 880 bytes
constexpr int C41H_POS = 6 * 9 * 3;                           // 162 positions per cube
constexpr int C41H_PIECES = 8 * 8 * 45 * 2;                   // 5 760 sixteen-byte pieces per cube

template <bool SLOPE01>
__global__ __launch_bounds__(512) void c3d2_conv41h_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem_c41[];
  unsigned* const reg = reinterpret_cast<unsigned*>(smem_c41);
  const int lane = threadIdx.x & 63, nt = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, kk = lane >> 4;
  u32x4 W[9][2][2];   // [tap][kb][H | L]
#pragma unroll
  for (int t = 0; t < 9; ++t) load_wblk(p.wblk, (nt * 9 + t) * 2, lane, W[t]);
  f32x4 b4, sl4;   // channels 16 nt + 4 kk .. + 3 of ONE position
  load_bias_slope(p.bias, p.slope, nt, kk, b4, sl4);
  const int n_items = p.n_utt;
  __shared__ int q_next;
  // piece e = t + 512 k (twelve per thread, 5 760 in all): run e / 90 = d * 8 + chunk, pixel (e % 90) / 2, channels 4 (e & 1) .. + 3
  constexpr int NPC = (C41H_PIECES + 511) / 512;
  f32x4 sv[NPC];
  auto load_item = [&](int it) {
    const float* const src = p.in + (int64_t)it * (8 * 8 * 45 * 8) + 4 * (int)threadIdx.x;
#pragma unroll
    for (int k = 0; k < NPC; ++k)
      if (k < NPC - 1 || threadIdx.x < C41H_PIECES - (NPC - 1) * 512) sv[k] = *reinterpret_cast<const f32x4*>(src + 2048 * k);
  };
  auto park_item = [&]() {
#pragma unroll
    for (int k = 0; k < NPC; ++k) {
      const int e = (int)threadIdx.x + 512 * k;
      const int run = (e * 46604) >> 22, r = e - 90 * run;        // e / 90 for e < 5 760
      const int d = run >> 3, chunk = run & 7;
      const int pix = r >> 1, ph = (pix * 13) >> 6, pw = pix - 5 * ph;       // pixel = 5 h + w; pix / 5 for pix < 45
      unsigned* const dst = reg + 4 * (chunk * C41H_PLANE + d * C41H_DP + 9 * pw + ph) + 2 * (r & 1);
      park_pieces(dst, 4 * 8 * C41H_PLANE, sv[k], k < NPC - 1 || threadIdx.x < C41H_PIECES - (NPC - 1) * 512);
    }
  };
  int item = blockIdx.x, item_next = item + (int)gridDim.x;   // the counter is drawn one item ahead, as in c3d2_conv32h_kernel
  if (item < n_items) {
    load_item(item);
    park_item();
  }
  __syncthreads();
  while (item < n_items) {
    unsigned q_ticket = 0;
    if (threadIdx.x == 0 && p.queue) q_ticket = atomicAdd(p.queue, 1u);
    if (item_next < n_items) load_item(item_next);
#pragma unroll 1
    for (int t = 0; t < (C41H_POS + 15) / 16; ++t) {
      const int P = min(16 * t + i, C41H_POS - 1);
      const int dq = (P * 2428) >> 16, r27 = P - 27 * dq;                       // P / 27 for P < 162;  r27 = 9 wq + h
      const int wq = (r27 * 7282) >> 16, h = r27 - 9 * wq;                      // r27 / 9 for r27 < 27
      // input pixel (dq + kd, h, wq + kw), channels 32 kb + 8 kk .. + 7: slot (dq + kd) * 59 + 9 (wq + kw) + h of plane 4 kb + kk [l: + 8]
      const char* const a2 = reinterpret_cast<const char*>(reg) + 16 * (kk * C41H_PLANE + dq * C41H_DP + r27);
      auto rd = [&](int st, int piece) -> u32x4 {   // step st = 2 tap + kb
        const int tap = st >> 1, kb = st & 1;
        return *reinterpret_cast<const u32x4*>(a2 + 16 * (C41H_DP * (tap / 3) + 9 * (tap % 3)) + 16 * 4 * C41H_PLANE * kb + 16 * 8 * C41H_PLANE * piece);
      };
      f32x4 a = b4;
      u32x4 bh[2], bl[2];
      bh[0] = rd(0, 0);
      bl[0] = rd(0, 1);
#pragma unroll
      for (int st = 0; st < 18; ++st) {
        if (st + 1 < 18) {
          bh[(st + 1) & 1] = rd(st + 1, 0);
          bl[(st + 1) & 1] = rd(st + 1, 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        a = mfma_pieces(W[st >> 1][st & 1][0], W[st >> 1][st & 1][1], bh[st & 1], bl[st & 1], a);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (16 * t + i < C41H_POS) {
        float* const o = p.out + ((((int64_t)item * 6 + dq) * 16 + 2 * nt + (kk >> 1)) * 27 + 3 * h + wq) * 8 + 4 * (kk & 1);
        *reinterpret_cast<f32x4*>(o) = prelu4<SLOPE01>(a, sl4);
      }
    }
    __syncthreads();   // nobody reads the planes any more
    if (item_next < n_items) park_item();
    if (threadIdx.x == 0) q_next = p.queue ? (int)q_ticket + 2 * (int)gridDim.x : item_next + (int)gridDim.x;
    __syncthreads();   // the next cube's planes are written
    item = item_next;
    item_next = q_next;
  }
}

// The launch of one persistent two-piece kernel (conv2_1 .. conv4_1): `p` with its work-item counter (from svk_work_queue, which the
// entry point has already called: a NULL queue = items at a fixed stride), the kernel of the pair that flags bit 1 selects, at most
// max_per_cu workgroups of `threads` per CU.  `name` is what the entry point's errors call the launch.
using ConvKernel = void (*)(const ConvParams);
int launch_conv(svk_ctx* ctx, const char* name, ConvKernel kern_slope01, ConvKernel kern_any, int32_t flags, ConvParams p, size_t lds,
                int threads, int max_per_cu, int64_t items, unsigned* queue) {
  const ConvKernel kern = (flags & 2) ? kern_slope01 : kern_any;
  p.queue = queue;
  unsigned grid;
  if (int rc = svk_persistent_grid(ctx, name, kern, lds, threads, max_per_cu, items, &grid)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

// The argument checks of svk_c3d2_stage2 .. svk_c3d2_conv41, in the order their errors are documented: the handle, n_utt, the
// flags, [nothing to do: n_utt = 0], NULL buffers (`all_set`), 16-byte alignment (`addr_bits`: the buffers' addresses or-ed) and
// the item index staying an int32: per_cube items per cube + the `ahead` grids of one workgroup per CU a ticket is drawn ahead.
// -> SVK_OK with *launch = whether there is anything to launch
int conv_checks(svk_ctx* ctx, int32_t n_utt, int32_t flags, bool all_set, uintptr_t addr_bits, int per_cube, int ahead, bool* launch) {
  *launch = false;
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n_utt >= 0, "n_utt negative");
  SVK_REQUIRE(ctx, (flags & ~2) == 0, "flags: only bit 1 (slopes in [0, 1]) is defined");
  if (n_utt == 0) return SVK_OK;
  SVK_REQUIRE(ctx, all_set, "NULL buffer");
  SVK_REQUIRE(ctx, (addr_bits & 15) == 0, "buffers must be 16-byte aligned");
  SVK_REQUIRE(ctx, (int64_t)n_utt * per_cube + ahead * (int64_t)ctx->num_cu < ((int64_t)1 << 31), "too many cubes for one launch");
  *launch = true;
  return SVK_OK;
}

// What differs between the one-layer entry points, and their common body
struct ConvEntry {
  const char* name;
  ConvKernel kern_slope01, kern_any;
  size_t lds;
  int threads, max_per_cu;
  int per_cube;   // work items per cube
  size_t slot;    // the kernel's work-item counter in the handle's scratch
  int ahead;      // grids its tickets are drawn ahead beyond the first (bounds the item index)
};
int conv_entry(svk_ctx* ctx, const ConvEntry& e, const float* d_in, int32_t n_utt, const void* d_wblk, const float* d_bias,
               const float* d_slope, int32_t flags, float* d_out) {
  bool launch;
  const uintptr_t addr_bits = reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_wblk) | reinterpret_cast<uintptr_t>(d_out);
  if (int rc = conv_checks(ctx, n_utt, flags, d_in && d_wblk && d_bias && d_slope && d_out, addr_bits, e.per_cube, e.ahead, &launch)) return rc;
  if (!launch) return SVK_OK;
  const ConvParams p{d_in, reinterpret_cast<const u32x4*>(d_wblk), d_bias, d_slope, d_out, n_utt, nullptr};
  unsigned* queue;
  if (int rc = svk_work_queue(ctx, e.slot, 1, &queue)) return rc;
  return launch_conv(ctx, e.name, e.kern_slope01, e.kern_any, flags, p, e.lds, e.threads, e.max_per_cu, (int64_t)n_utt * e.per_cube, queue);
}

}  // namespace

extern "C" int svk_c3d2_stage2(svk_ctx* ctx, const float* d_in, int32_t n_utt, const void* d_w21blk,
                               const float* d_bias21, const float* d_slope21, const void* d_w22blk,
                               const float* d_bias22, const float* d_slope22, int32_t flags, float* d_act2, float* d_out) {
  bool launch;
  const uintptr_t addr_bits = reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_act2) | reinterpret_cast<uintptr_t>(d_w21blk) |
                              reinterpret_cast<uintptr_t>(d_w22blk) | reinterpret_cast<uintptr_t>(d_out);
  // SVK_C3D2_STAGE2_TWO_KERNELS (read at every call) selects c3d2_conv21h_kernel + c3d2_conv22h_kernel through d_act2: the reference
  // the streamed kernel is tested and measured against, not a second shipped path.  The streamed kernel never touches d_act2.
  const bool two_kernels = getenv("SVK_C3D2_STAGE2_TWO_KERNELS") != nullptr;
  if (int rc = conv_checks(ctx, n_utt, flags,
                           d_in && d_w21blk && d_bias21 && d_slope21 && d_w22blk && d_bias22 && d_slope22 && (d_act2 || !two_kernels) && d_out,
                           addr_bits, 21, 0, &launch))
    return rc;
  if (!launch) return SVK_OK;
  if (!two_kernels) {
    using Stage2Kernel = void (*)(const Stage2Params);
    const Stage2Kernel kern = (flags & 2) ? c3d2_stage2h_kernel<true> : c3d2_stage2h_kernel<false>;
    Stage2Params p{d_in, reinterpret_cast<const u32x4*>(d_w21blk), d_bias21, d_slope21, reinterpret_cast<const u32x4*>(d_w22blk), d_bias22,
                   d_slope22, d_out, n_utt, nullptr};
    if (int rc = svk_work_queue(ctx, SVK_SLOT_STAGE2, 1, &p.queue)) return rc;
    // (svk_persistent_grid allows 64 bytes of static LDS beside the dynamic region; this kernel has S2S_STATIC_LDS: checked here)
    static_assert(sizeof(unsigned) * (size_t)S2S_LDS_WORDS + S2S_STATIC_LDS <= 160 * 1024, "one workgroup must fit a CU's LDS");
    if (sizeof(unsigned) * (size_t)S2S_LDS_WORDS + S2S_STATIC_LDS > (size_t)ctx->lds_per_cu)
      return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "svk_c3d2_stage2 needs %zu bytes of LDS per workgroup (device: %d)",
                      sizeof(unsigned) * (size_t)S2S_LDS_WORDS + S2S_STATIC_LDS, ctx->lds_per_cu);
    unsigned grid;
    if (int rc = svk_persistent_grid(ctx, "svk_c3d2_stage2", kern, sizeof(unsigned) * (size_t)S2S_LDS_WORDS, 512, 1, (int64_t)n_utt * O2_W, &grid))
      return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), sizeof(unsigned) * (size_t)S2S_LDS_WORDS, ctx->stream, p);
    SVK_LAUNCH_CHECK(ctx);
    return SVK_OK;
  }
  // conv2_1 and conv2_2 share a CU between workgroups: as many as the occupancy calculator allows
  unsigned* queues;
  if (int rc = svk_work_queue(ctx, SVK_SLOT_STAGE2, 2, &queues)) return rc;
  const ConvParams p21{d_in, reinterpret_cast<const u32x4*>(d_w21blk), d_bias21, d_slope21, d_act2, n_utt, nullptr};
  if (int rc = launch_conv(ctx, "svk_c3d2_stage2 (conv2_1)", c3d2_conv21h_kernel<true>, c3d2_conv21h_kernel<false>, flags, p21,
                           sizeof(unsigned) * (size_t)C21H_LDS_WORDS, 256, INT_MAX, (int64_t)n_utt * (S2_H / 4), queues))
    return rc;
  const ConvParams p22{d_act2, reinterpret_cast<const u32x4*>(d_w22blk), d_bias22, d_slope22, d_out, n_utt, nullptr};
  return launch_conv(ctx, "svk_c3d2_stage2 (conv2_2)", c3d2_conv22h_kernel<true>, c3d2_conv22h_kernel<false>, flags, p22,
                     sizeof(unsigned) * (size_t)C22H_LDS_WORDS, 256, INT_MAX, (int64_t)n_utt * 21, queues ? queues + 1 : nullptr);
}

extern "C" int svk_c3d2_conv31(svk_ctx* ctx, const float* d_in, int32_t n_utt, const void* d_wblk, const float* d_bias,
                               const float* d_slope, int32_t flags, float* d_out) {
  static const ConvEntry e{"svk_c3d2_conv31", c3d2_conv31h_kernel<true>, c3d2_conv31h_kernel<false>, sizeof(unsigned) * (size_t)C31H_LDS_WORDS,
                           256, INT_MAX, 5, SVK_SLOT_CONV31, 0};
  return conv_entry(ctx, e, d_in, n_utt, d_wblk, d_bias, d_slope, flags, d_out);
}

extern "C" int svk_c3d2_conv32t(svk_ctx* ctx, const float* d_in, int32_t n_utt, const void* d_wblk, const float* d_bias,
                                const float* d_slope, int32_t flags, float* d_out) {
  static const ConvEntry e{"svk_c3d2_conv32t", c3d2_conv32h_kernel<true>, c3d2_conv32h_kernel<false>,
                           sizeof(float) * (size_t)(C32H_LDS_WORDS + C32H_XCH_FLOATS), 512, 1, 5, SVK_SLOT_CONV32, 2};
  return conv_entry(ctx, e, d_in, n_utt, d_wblk, d_bias, d_slope, flags, d_out);
}

extern "C" int svk_c3d2_conv41(svk_ctx* ctx, const float* d_in, int32_t n_utt, const void* d_wblk, const float* d_bias,
                               const float* d_slope, int32_t flags, float* d_out) {
  static const ConvEntry e{"svk_c3d2_conv41", c3d2_conv41h_kernel<true>, c3d2_conv41h_kernel<false>, sizeof(unsigned) * (size_t)C41H_LDS_WORDS,
                           512, 1, 1, SVK_SLOT_CONV41, 2};
  return conv_entry(ctx, e, d_in, n_utt, d_wblk, d_bias, d_slope, flags, d_out);
}
