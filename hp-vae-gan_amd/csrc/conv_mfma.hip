// 3x3 / 3x3x3 "same" convolution as an implicit GEMM on the gfx950 fp32 matrix cores.
//
// Replaces (reference, /root/reference): nn.Conv3d / nn.Conv2d forward as used by
//   ConvBlock3D       modules/networks_3d.py:48-56     ConvBlock2D   modules/networks_2d.py:53-61
//   ConvBlock3DSN     modules/networks_3d.py:59-70     ConvBlock2DSN modules/networks_2d.py:64-75
//   tails             modules/networks_3d.py:175,341,362
// and, through a flipped/transposed weight pack, their backward-data pass (stride 1, pad 1:
// bwd-data is a forward conv with W'[c][o][tap] = W[o][c][ntaps-1-tap]).
//
// GEMM view (per batch sample b and output time-plane t):
//     Y[o][q] = sum_{tap} sum_{c} W[o][c][tap] * X[c][q + off(tap)]
//   M = output channels (32 per MFMA tile, MB tiles per wave)
//   N = output positions q of one (Th x Tw) spatial tile, flattened with the LDS row stride
//       RS = Tw + 2 so that every tap is a constant offset (the two halo columns per row yield
//       junk columns of the GEMM that are never stored)
//   K = (tap, input-channel) - two input channels per v_mfma_f32_32x32x2_f32.
//
// Data movement: the input tile (CC channels x KT time planes x (Th+2) x (Tw+2), zero padded) is
// staged through LDS one channel chunk at a time (LDS-DMA; register staged when the producer's
// BatchNorm-apply + LeakyReLU is fused into the load); the B operand is read with
// conflict-free ds_read_b32 (32 consecutive dwords per half wave).  The A operand (weights) is
// pre-packed in fragment order and read straight from L2 with one 16-byte load per lane per
// (tap, m-tile); all workgroups read the same 442 KB so it stays L2 resident.
// Accumulation is exact fp32 (v_mfma_f32_32x32x2_f32 == chain of fmaf).
#include "hpvg_common.h"
#include "hpvg_host.h"
#include "hpvg.h"
#include <stdlib.h>

namespace {

// source of zero padding for the LDS-DMA staging (out-of-image lanes read this word)
__device__ const float g_zero_word[16] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
// a whole H x W plane of zeros (conv_wino2r_kernel: a time plane outside the clip is staged like any other, from here)
constexpr long HPVG_ZERO_PLANE_FLOATS = 1L << 18;
__device__ float g_zero_plane[HPVG_ZERO_PLANE_FLOATS];

#ifdef HPVG_TRACE
// development build only (tools/trace_conv.py): per-workgroup start/end (100 MHz clock) and placement
__device__ unsigned long long g_trace[8192 * 4];
__device__ unsigned long long g_phase[8192 * 4];  // per workgroup (wave 0): cycles issuing DMA, waiting for it, in the MFMA loop, epilogue
#define HPVG_PH(i) { unsigned long long now_ = __builtin_readcyclecounter(); ph_a[i] += now_ - ph_t; ph_t = now_; }
#define HPVG_PH_INIT unsigned long long ph_t = __builtin_readcyclecounter(); unsigned long long ph_a[4] = {0, 0, 0, 0};
#define HPVG_PH_END if (threadIdx.x == 0) { for (int i_ = 0; i_ < 4; ++i_) g_phase[4 * blockIdx.x + i_] = ph_a[i_]; }
#define HPVG_TRACE_BEGIN unsigned long long tr_t0 = wall_clock64(); unsigned long long tr_c0 = __builtin_readcyclecounter();
#define HPVG_TRACE_END                                                              \
  if (threadIdx.x == 0 && blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z) < 8192) { \
    unsigned long long* tr = g_trace + 4 * (blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)); \
    tr[0] = tr_t0;                                                                  \
    tr[1] = wall_clock64();                                                         \
    tr[2] = __builtin_amdgcn_s_getreg((31 << 11) | 4);                              \
    tr[3] = (__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xF) | ((__builtin_readcyclecounter() - tr_c0) << 8); \
  }
#else
#define HPVG_TRACE_BEGIN
#define HPVG_TRACE_END
#define HPVG_PH(i)
#define HPVG_PH_INIT
#define HPVG_PH_END
#endif

struct ConvFwdArgs {
  const float* x;
  const float* wp;
  const float* bias;
  const float* in_scale;
  const float* in_shift;
  const float* mask;  // optional [B][Cout][T][H][W]: y *= (mask > 0 ? 1 : 0.2) - leaky_relu_backward fused into the backward-data conv
  // 1-bit form of such a mask, [B][T*H*W][ceil(Cout/32)] words (bit c%32 of word c/32 = activation > 0):
  const unsigned* mask_bits;  // read by the masked epilogue INSTEAD of `mask` when given (8 loads per tile and lane, not 128)
  unsigned* bits_out;         // written by a LeakyReLU epilogue for its consumer's backward-data conv
  float* y;
  int B, Cin, Cout, T, H, W;
  // tile = `L` consecutive positions of the row-flattened band (W split into ntw bands of Tw columns, LDS row stride
  // RS = Tw + 2), nrange tiles per band and plane; Th only for the 2-D tiles of the narrow kernel (L = Th * RS)
  int Th, Tw, RS, PL, L, qstride, nrange, ntw, nblocks, nchunk, mbtot, nj;  // tile r of a band starts at r * qstride
  int in_lrelu, out_lrelu;
  // schedule: tiles [0, ndp*S) are data-parallel rounds (round k: tile k*S + g), tiles [skbase, ntl) are cut into
  // (tile, channel-chunk) items dealt evenly over the S workgroups (stream-K)
  int gridy, ntl, ndp, skbase;
  float* skpart;  // [S][2][MB*NB*16][256] raw accumulator slabs of partially computed tiles
  int stagger;    // conv_wino_kernel: the workgroup in a CU's odd wave slot starts this many s_sleep(127) (~4 us each) late
};

template <int CP> struct AVecT;
template <> struct AVecT<4> { typedef f32x4 type; };
template <> struct AVecT<2> { typedef f32x2 type; };

constexpr int NJMAX = 4;  // (Th+2)*RS <= 1024

// ------------------------------------------------------------------------------------------
// Schedule (stream-K).  A workgroup's serial K loop over one tile (8 chunks x 864 MFMAs per wave) lasts ~200 us, so a
// grid of one workgroup per tile with 1-5 tiles per CU slot is badly quantised (2080 tiles on 512 slots: the fifth
// round is 6 % full; 560 tiles: the second round 9 %).  The grid is therefore exactly the number of co-resident
// workgroups S (2 per CU, 512).  Tiles [0, ndp*S) are handed out whole (round k: tile k*S + g); the remaining tiles
// are cut into (tile, channel chunk) items and the item list is split evenly over the S workgroups, so every
// workgroup runs the same number of chunk iterations +-1.  A tile whose chunks end up in more than one workgroup is
// written as raw accumulator slabs (register order, fully coalesced) and finished by conv_fixup_kernel in workgroup
// order (reproducible; no float atomics).  With S = number of tiles the same kernel is the plain one-workgroup-per-tile
// launch (no workspace needed).
// Measured on MI355X (tools/trace_conv.py, per-workgroup timeline): one workgroup per CU already saturates the matrix
// pipe (2 per CU: +3 %); the sustained shader clock under this load is 2.03-2.07 GHz with real data (2.29 GHz when the
// operands are zeros), i.e. the fp32 MFMA ceiling of the part is ~134 TFLOP/s, not the 157.3 of 2.4 GHz.
struct SkTile { int b, t, q0, w0, mb0; };
__device__ __forceinline__ SkTile sk_decode_tile(const ConvFwdArgs& a, int tile, int MB) {
  SkTile c;
  // tile order: output-channel group fastest, then TIME, then the spatial tile.  Consecutive ids (= one XCD, thanks to
  // hpvg_xcd_remap) are then the same spatial tile at neighbouring t: the input planes t-1, t, t+1 they share are fetched
  // from HBM once and hit in that XCD's L2 for the other two (spatial-major order re-read every plane 3x: PMC)
  const int yb = tile % a.gridy;
  int r = tile / a.gridy;
  c.t = r % a.T; r /= a.T;
  const int tw_i = r % a.ntw; r /= a.ntw;
  const int r_i = r % a.nrange;
  c.b = r / a.nrange;
  c.q0 = r_i * a.qstride;
  c.w0 = tw_i * a.Tw;
  c.mb0 = yb * MB;
  return c;
}

// Per-thread staging slots of a tile: position p = j*256+tid inside one (Th+2) x RS input plane (zero padded).
struct StageSlots {
  int gofs[NJMAX];        // element offset inside a (c,t) plane (valid lanes)
  unsigned bofs[NJMAX];   // the same in bytes (planes are < 4 GB)
  unsigned okmask, wmask; // bit j: slot j lies inside the image / inside the staged plane
  unsigned long long em[NJMAX];  // EXEC mask of the lanes whose slot j lies inside the image (wave-uniform)
};
__device__ __forceinline__ StageSlots conv_stage_slots(const ConvFwdArgs& a, int q0, int w0, int tid) {
  // slot p holds position P = q0 + p of the zero-padded, row-flattened band: row P / RS - 1, column w0 + P % RS - 1
  StageSlots sl;
  sl.okmask = 0;
  sl.wmask = 0;
  const int RS = a.RS, plload = a.L + 2 * RS + 2;
#pragma unroll
  for (int j = 0; j < NJMAX; ++j) {
    const int p = j * 256 + tid;
    sl.gofs[j] = 0;
    sl.bofs[j] = 0;
    if (j < a.nj && p < plload) {
      const int P = q0 + p;
      const int hh = P / RS, ww = P - hh * RS;
      const int gh = hh - 1, gw = w0 + ww - 1;
      sl.wmask |= 1u << j;
      if (gh >= 0 && gh < a.H && gw >= 0 && gw < a.W) {
        sl.okmask |= 1u << j;
        sl.gofs[j] = gh * a.W + gw;
        sl.bofs[j] = (unsigned)sl.gofs[j] * 4u;
      }
    }
    sl.em[j] = __ballot((sl.okmask >> j) & 1u);
  }
  return sl;
}

#ifndef HPVG_CONV_ASM_STAGE
#define HPVG_CONV_ASM_STAGE 1
#endif
// One LDS-DMA piece of the staging loop as straight-line code: scalar plane base + per-lane byte offset (no address
// VALU), the out-of-image lanes switched off through EXEC inside the statement (the builtin under `if (lane ok)` is a
// saveexec + taken branch + a 64-bit VALU add per piece).  Invisible to the compiler: the barrier that publishes the chunk is
// preceded by an explicit s_waitcnt vmcnt(0).
__device__ __forceinline__ void conv_dma_piece(const char* base_, unsigned voff, unsigned lds_addr, unsigned long long mask) {
  // the base IS wave-uniform, but under SGPR pressure hipcc may keep it in VGPRs and then hands the asm statement a VGPR
  // pair for its "s" operand (an assembler error at best): rebuild it from two readfirstlanes so that its definition is scalar
  const unsigned long long bb = (unsigned long long)base_;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)bb);            // (the builtin returns int:
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(bb >> 32));    //  no sign extension, please)
  const unsigned long long base = (unsigned long long)lo | ((unsigned long long)hi << 32);
  unsigned long long keep_exec;
  unsigned keep_m0;
  asm volatile(
      "s_mov_b64 %0, exec\n\t"
      "s_mov_b32 %1, m0\n\t"
      "s_mov_b64 exec, %3\n\t"
      "s_mov_b32 m0, %4\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %2, %5\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_mov_b64 exec, %0"
      : "=&s"(keep_exec), "=&s"(keep_m0)
      : "v"(voff), "s"(mask), "s"(lds_addr), "s"(base)
      : "memory");
}

// The same for a 16-byte piece (global_load_lds_dwordx4: LDS destination = m0 + 16 * lane).  Neither the per-lane global
// address nor the LDS base needs more than 4-byte alignment (tools/glds16_probe.hip, run on MI355X: correct for every
// source and destination offset, no measurable cost).
__device__ __forceinline__ void conv_dma_piece16(const char* base_, unsigned voff, unsigned lds_addr, unsigned long long mask) {
  const unsigned long long bb = (unsigned long long)base_;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)bb);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(bb >> 32));
  const unsigned long long base = (unsigned long long)lo | ((unsigned long long)hi << 32);
  unsigned long long keep_exec;
  unsigned keep_m0;
  asm volatile(
      "s_mov_b64 %0, exec\n\t"
      "s_mov_b32 %1, m0\n\t"
      "s_mov_b64 exec, %3\n\t"
      "s_mov_b32 m0, %4\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %2, %5\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_mov_b64 exec, %0"
      : "=&s"(keep_exec), "=&s"(keep_m0)
      : "v"(voff), "s"(mask), "s"(lds_addr), "s"(base)
      : "memory");
}

// The 16-byte piece for call sites where EVERY lane of the wave is active (the K loops): EXEC goes back to all ones by
// constant and m0 is declared clobbered instead of saved and restored - measured with tools/mfma_fillers.hip, a vector-memory
// instruction between two fp32 MFMAs costs the matrix pipe ~40 cycles whatever its width or its active lanes, and the
// save / restore pairs another 16 (the restoring s_mov of m0 and of exec each delay the MFMA behind them); this form: 47.
__device__ __forceinline__ void conv_dma_piece16_all(const char* base_, unsigned voff, unsigned lds_addr, unsigned long long mask) {
  const unsigned long long bb = (unsigned long long)base_;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)bb);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(bb >> 32));
  const unsigned long long base = (unsigned long long)lo | ((unsigned long long)hi << 32);
  asm volatile(
      "s_mov_b64 exec, %1\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %3\n\t"
      "s_mov_b64 exec, -1"
      :
      : "v"(voff), "s"(mask), "s"(lds_addr), "s"(base)
      : "memory", "m0");
}

// Stage channel chunk `ch` (CC channels x KT time planes) of the tile of sample b / output plane t into xs.
template <int CC, int KT, bool PRO>
__device__ __forceinline__ void conv_stage_chunk(const ConvFwdArgs& a, float* xs, const StageSlots& sl, int ch, bool first_chunk,
                                                 int b, int t, int tid, int wave) {
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  const long HW = (long)a.H * a.W;
  const int PL = a.PL;
  if constexpr (!PRO) {
    // LDS-DMA staging with as little VALU work as possible (a co-resident wave with MFMAs queued keeps the SIMD's
    // VALU port busy, which stretched a select-per-load version of this loop from 2.4 to 15-20 us per chunk): the
    // per-lane byte offsets are tile constants, the plane base is scalar, out-of-image lanes are switched off by
    // EXEC and their LDS words are zeroed once per tile (no load ever writes them).
    // plane pointers advance by scalar adds (recomputing ((b*Cin + c)*T + t)*HW per plane is ~15 scalar instructions of
    // 64-bit multiply in a loop whose pieces cost ~8)
    const long HWb = HW * 4;
    const char* cbase = reinterpret_cast<const char*>(a.x) + (((long)b * a.Cin + (long)ch * CC) * a.T + (t - (KT == 3 ? 1 : 0))) * HWb;
    int pl = 0;
#pragma unroll 1
    for (int c = 0; c < CC; ++c, cbase += (long)a.T * HWb)
#pragma unroll
    for (int dt = 0; dt < KT; ++dt, ++pl) {
      const int cg = ch * CC + c;
      const int tt = t + dt - (KT == 3 ? 1 : 0);
      const bool valid = cg < a.Cin && tt >= 0 && tt < a.T;
      float* dst = xs + pl * PL + wave * 64;
      if (valid) {
        const char* src = cbase + dt * HWb;
#if HPVG_CONV_ASM_STAGE
        const unsigned dst_lds = (unsigned)(size_t)(lptr_t)dst;
#pragma unroll
        for (int j = 0; j < NJMAX; ++j)
          if (sl.em[j] != 0ull) conv_dma_piece(src, sl.bofs[j], dst_lds + j * 1024, sl.em[j]);
#else
#pragma unroll
        for (int j = 0; j < NJMAX; ++j)
          if ((sl.okmask >> j) & 1u)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + sl.bofs[j]), (lptr_t)(dst + j * 256), 4, 0, 0);
#endif
        if (first_chunk) {
#pragma unroll
          for (int j = 0; j < NJMAX; ++j)
            if (((sl.wmask & ~sl.okmask) >> j) & 1u) xs[pl * PL + j * 256 + tid] = 0.f;
        }
      } else if (first_chunk || cg >= a.Cin) {
        // a plane outside the clip (t) stays zero for the whole tile; a channel past Cin only exists in the last chunk
#pragma unroll
        for (int j = 0; j < NJMAX; ++j)
          if ((sl.wmask >> j) & 1u) xs[pl * PL + j * 256 + tid] = 0.f;
      }
    }
  } else {
    // through registers: the producer's BatchNorm-apply (+ LeakyReLU) is fused into the load
#pragma unroll 2
    for (int c = 0; c < CC; ++c) {
      const int cg = ch * CC + c;
      const bool cok = cg < a.Cin;
      float sc = 1.f, sh = 0.f;
      if (cok) {
        sc = a.in_scale[cg];
        sh = a.in_shift[cg];
      }
      float v[KT][NJMAX];
#pragma unroll
      for (int dt = 0; dt < KT; ++dt) {
        const int tt = t + dt - (KT == 3 ? 1 : 0);
        const bool tok = cok && tt >= 0 && tt < a.T;
        const float* src = a.x + (((long)b * a.Cin + (cok ? cg : 0)) * a.T + (tok ? tt : 0)) * HW;
#pragma unroll
        for (int j = 0; j < NJMAX; ++j) {
          const bool ld = tok && ((sl.okmask >> j) & 1u);
          v[dt][j] = ld ? src[sl.gofs[j]] : 0.f;
        }
      }
#pragma unroll
      for (int dt = 0; dt < KT; ++dt) {
        const int tt = t + dt - (KT == 3 ? 1 : 0);
        const bool tok = cok && tt >= 0 && tt < a.T;
#pragma unroll
        for (int j = 0; j < NJMAX; ++j) {
          if ((sl.wmask >> j) & 1u) {
            float val = v[dt][j];
            if (tok && ((sl.okmask >> j) & 1u)) {
              val = val * sc + sh;
              if (a.in_lrelu) val = hpvg_lrelu(val);
            }
            xs[(c * KT + dt) * PL + j * 256 + tid] = val;
          }
        }
      }
    }
  }
}

// Co-resident workgroups per CU.  Default: two (256 VGPRs each).  Development build -DHPVG_CONV_WGS4: instances with at
// most 4 accumulator tiles per wave (64 accumulator registers) are compiled for FOUR per CU (<= 128 VGPRs, LDS <= 38 KB)
// - more workgroups staging while others own the matrix pipe (tools/ab_conv_wgs.py: the A/B).
#ifdef HPVG_CONV_WGS4
#define HPVG_CONV_WGS(MB, NB) ((MB) * (NB) <= 4 ? 4 : 2)
#else
#define HPVG_CONV_WGS(MB, NB) 2
#endif

// VAR selects what is compiled around the MFMA loop, so that the plain instance - every forward conv and most backward-data
// convs of the path - carries none of it (a run-time `if (a.mask)` in the epilogue alone cost the plain launches +1.6 % at
// stage 9 through register allocation): 0 = plain, 1 = out_mask epilogue (leaky_relu_backward of the layer below),
// 2 = the producer's BatchNorm-apply (+ LeakyReLU) fused into the staging (register path instead of LDS-DMA).
constexpr int VAR_PLAIN = 0, VAR_MASK = 1, VAR_PRO = 2, VAR_BITS = 3;   // 3 = plain + bits_out (the activated forward convs)

template <int CC, int KT, int MB, int NB, int VAR>
__global__ __launch_bounds__(256, HPVG_CONV_WGS(MB, NB)) void conv_mfma_kernel(const ConvFwdArgs a) {
  constexpr int CP = CC / 2;
  constexpr int TAPS = KT * 9;
  typedef typename AVecT<CP>::type AVec;
  extern __shared__ __attribute__((aligned(16))) float xs[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const long HW = (long)a.H * a.W;
  const int RS = a.RS, PL = a.PL;
  const float* xl = xs + half * KT * PL + l31 + wave * 32;

  HPVG_TRACE_BEGIN
  const int S = gridDim.x;
  const int g = hpvg_xcd_remap(blockIdx.x, S);
  const long Isk = (long)(a.ntl - a.skbase) * a.nchunk;
  int it = (int)((long)g * Isk / S);
  const int it_hi = (int)((long)(g + 1) * Isk / S);
  const int first_sk_tile = a.skbase + it / a.nchunk;

  HPVG_PH_INIT
  bool first_stage = true;
  for (int k = 0;; ++k) {
    int tile, ch_lo, ch_hi;
    if (k < a.ndp) {
      tile = k * S + g;
      ch_lo = 0;
      ch_hi = a.nchunk;
    } else {
      if (it >= it_hi) break;
      const int tr = it / a.nchunk;
      tile = a.skbase + tr;
      ch_lo = it - tr * a.nchunk;
      const int n = (a.nchunk - ch_lo < it_hi - it) ? a.nchunk - ch_lo : it_hi - it;
      ch_hi = ch_lo + n;
      it += n;
    }
    const SkTile tc = sk_decode_tile(a, tile, MB);
    const int b = tc.b, t = tc.t, q0 = tc.q0, w0 = tc.w0, mb0 = tc.mb0;

    const StageSlots sl = conv_stage_slots(a, q0, w0, tid);

    f32x16 acc[MB][NB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][i][e] = 0.f;

    for (int ch = ch_lo; ch < ch_hi; ++ch) {
      if (!first_stage) __syncthreads();  // every wave is done reading the previous chunk
      first_stage = false;
      HPVG_PH(3)
      // Retire every outstanding vector-memory write to a VGPR (the A prefetch issued past the previous chunk's last tap
      // is never consumed) BEFORE the staging loop: the loop reuses those registers for addresses, and a write-after-
      // write hazard the compiler cannot count across the loop's back edge costs an s_waitcnt vmcnt(0) per DMA, i.e.
      // serialises all 72 loads of the chunk (measured: 1.98 -> 2.22 ms at stage 9).
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      conv_stage_chunk<CC, KT, VAR == VAR_PRO>(a, xs, sl, ch, ch == ch_lo, b, t, tid, wave);
      HPVG_PH(0)
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the asm LDS-DMA pieces are invisible to the compiler's counters
      __syncthreads();
      HPVG_PH(1)

      const AVec* wpt = reinterpret_cast<const AVec*>(a.wp) + ((long)(ch * TAPS) * a.mbtot + mb0) * 64 + lane;
      AVec av[MB];
#pragma unroll
      for (int m = 0; m < MB; ++m) av[m] = wpt[m * 64];
      float bv[2][NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) bv[0][i] = xl[i * 128];
#pragma unroll 1
      for (int dt = 0; dt < KT; ++dt) {
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
#pragma unroll
          for (int dw = 0; dw < 3; ++dw) {
            wpt += (long)a.mbtot * 64;
            AVec an[MB];
#pragma unroll
            for (int m = 0; m < MB; ++m) an[m] = wpt[m * 64];
            const float* xt = xl + dt * PL + dh * RS + dw;
            const float* xn = (dw < 2) ? xt + 1 : (dh < 2 ? xl + dt * PL + (dh + 1) * RS : xl + (dt + 1 < KT ? dt + 1 : 0) * PL);
#pragma unroll
            for (int cp = 0; cp < CP; ++cp) {
              const float* nx = (cp + 1 < CP) ? xt + (2 * (cp + 1) * KT) * PL : xn;
#pragma unroll
              for (int i = 0; i < NB; ++i) bv[(cp + 1) & 1][i] = nx[i * 128];
              __builtin_amdgcn_sched_barrier(0);
              __builtin_amdgcn_s_setprio(1);
#pragma unroll
              for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int m = 0; m < MB; ++m)
                  acc[m][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][cp], bv[cp & 1][i], acc[m][i], 0, 0, 0);
              __builtin_amdgcn_s_setprio(0);
            }
#pragma unroll
            for (int m = 0; m < MB; ++m) av[m] = an[m];
          }
        }
      }
      HPVG_PH(2)
    }

    if (ch_lo != 0 || ch_hi != a.nchunk) {
      // ---- part of a tile: raw accumulators, register order (each store instruction writes 256 contiguous bytes)
      const int seg = (tile == first_sk_tile) ? 0 : 1;
      float* dst = a.skpart + ((long)(g * 2 + seg) * (MB * NB * 16)) * 256 + tid;
#pragma unroll
      for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) dst[((m * NB + i) * 16 + e) * 256] = acc[m][i][e];
      continue;
    }
    // ---- whole tile: bias (added AFTER the accumulation, as every torch conv backend does: a BatchNorm fed by a
    // nearly constant channel amplifies the difference between (bias + sum) and (sum + bias) to percent level),
    // optional LeakyReLU, masked store
    float bias_r[MB][16];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = (mb0 + m) * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
        bias_r[m][e] = (a.bias && co < a.Cout) ? a.bias[co] : 0.f;
      }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int blk = wave + 4 * i;
      const int q = blk * 32 + l31;
      const int Q = q0 + q;
      const int gh = Q / RS, ww = Q - gh * RS;
      const int gw = w0 + ww;
      const bool ok = q < a.L && ww < a.Tw && gh < a.H && gw < a.W;
      const long sp = (long)t * HW + (long)gh * a.W + gw;
      const long wi = ((long)b * a.mbtot + mb0) * a.T * HW + sp;   // mask word of this position, m-tile mb0; m-tile + m: + m * T*H*W
      if constexpr (VAR == VAR_BITS) {
        // (every lane takes part in the cross-half exchange below, so no early exit before it)
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          unsigned word = 0;
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float val = acc[m][i][e] + bias_r[m][e];      // sign(LeakyReLU(v)) = sign(v)
            word |= (val > 0.f ? 1u : 0u) << ((e & 3) + 8 * (e >> 2) + 4 * half);
          }
          word |= (unsigned)__shfl_xor((int)word, 32, 64);      // the two half-waves hold complementary channels of one position
          if (ok && half == 0 && (mb0 + m) * 32 < a.Cout) a.bits_out[wi + (long)m * a.T * HW] = word;
        }
      }
      if (!ok) continue;
      unsigned mword[MB];
      if constexpr (VAR == VAR_MASK) {
        if (a.mask_bits) {
#pragma unroll
          for (int m = 0; m < MB; ++m) mword[m] = (mb0 + m) * 32 < a.Cout ? a.mask_bits[wi + (long)m * a.T * HW] : 0u;
        }
      }
#pragma unroll
      for (int m = 0; m < MB; ++m) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int co = (mb0 + m) * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
          if (co < a.Cout) {
            float val = acc[m][i][e] + bias_r[m][e];
            if (a.out_lrelu) val = hpvg_lrelu(val);
            const long oi = ((long)b * a.Cout + co) * a.T * HW + sp;
            if constexpr (VAR == VAR_MASK) {
              if (a.mask_bits) val *= ((mword[m] >> ((e & 3) + 8 * (e >> 2) + 4 * half)) & 1u) ? 1.f : HPVG_LRELU_SLOPE;
              else val *= a.mask[oi] > 0.f ? 1.f : HPVG_LRELU_SLOPE;
            }
            a.y[oi] = val;
          }
        }
      }
    }
  }
  HPVG_PH_END
  HPVG_TRACE_END
}

// Finishes the tiles conv_mfma_kernel computed in parts: one workgroup per stream-K tile, partial slabs summed in
// workgroup order, then the same epilogue.  Tiles computed whole by one workgroup were already stored: nothing to do.
__global__ __launch_bounds__(256) void conv_fixup_kernel(const ConvFwdArgs a, int S, int MB, int NB) {
  const int r = blockIdx.x;                   // stream-K tile
  const int mi = blockIdx.y;                  // (m-tile, position block) of the accumulator slab
  const int m = mi / NB, i = mi - m * NB;
  const long Isk = (long)(a.ntl - a.skbase) * a.nchunk;
  const long i0 = (long)r * a.nchunk, i1 = i0 + a.nchunk - 1;
  const int g0 = (int)(((i0 + 1) * S + Isk - 1) / Isk) - 1;  // owner of the tile's first item
  const int g1 = (int)(((i1 + 1) * S + Isk - 1) / Isk) - 1;  // ... and of its last
  if (g0 == g1) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const SkTile tc = sk_decode_tile(a, a.skbase + r, MB);
  const long HW = (long)a.H * a.W;
  const int RS = a.RS;
  const int blk = wave + 4 * i;
  const int q = blk * 32 + l31;
  const int Q = tc.q0 + q;
  const int gh = Q / RS, ww = Q - gh * RS;
  const int gw = tc.w0 + ww;
  if (!(q < a.L && ww < a.Tw && gh < a.H && gw < a.W)) return;
  const long slab = (long)MB * NB * 16 * 256;
  float v[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = 0.f;
  for (int g = g0; g <= g1; ++g) {
    const long st = (long)g * Isk / S, en = (long)(g + 1) * Isk / S;
    if (st == en) continue;  // workgroup without stream-K items
    const int seg = (st / a.nchunk == r) ? 0 : 1;
    const float* src = a.skpart + (long)(g * 2 + seg) * slab + (long)mi * 16 * 256 + tid;
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] += src[e * 256];
  }
  const long sp = (long)tc.t * HW + (long)gh * a.W + gw;
  const long wi = ((long)tc.b * a.mbtot + tc.mb0 + m) * a.T * HW + sp;
  const unsigned mword = a.mask_bits ? a.mask_bits[wi] : 0u;
  unsigned word = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int co = (tc.mb0 + m) * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
    if (co >= a.Cout) continue;
    float val = v[e];
    if (a.bias) val += a.bias[co];
    word |= (val > 0.f ? 1u : 0u) << ((e & 3) + 8 * (e >> 2) + 4 * half);
    if (a.out_lrelu) val = hpvg_lrelu(val);
    const long oi = ((long)tc.b * a.Cout + co) * a.T * HW + sp;
    if (a.mask_bits) val *= ((mword >> ((e & 3) + 8 * (e >> 2) + 4 * half)) & 1u) ? 1.f : HPVG_LRELU_SLOPE;
    else if (a.mask) val *= a.mask[oi] > 0.f ? 1.f : HPVG_LRELU_SLOPE;
    a.y[oi] = val;
  }
  if (a.bits_out) {
    // the partner half-wave holds the other 16 channels of this position; lanes that returned early above belong to
    // positions outside the tile in BOTH halves (the test does not depend on `half`), so the exchange is well defined
    word |= (unsigned)__shfl_xor((int)word, 32, 64);
    if (half == 0) a.bits_out[wi] = word;
  }
}

#include "conv_wino.inl"
#include "conv_wino2d.inl"
#include "conv_wino2r.inl"

// ------------------------------------------------------------------------------------------
// Narrow-output convolution (Cout <= 4): the tails 64->3 / 64->1 (networks_3d.py:175,341,362) and the backward-data
// pass of the 3->64 heads.  With output channels as the GEMM's M these waste >= 90 % of every 32-row tile (1.07 ms at
// stage 9).  Here the roles are swapped and the 9 in-plane taps move into N:
//     P[pos][(o,dh,dw)] = sum_{c,dt} x[c][t+dt-pt][pos] * w[o][c][dt][dh][dw]          (GEMM: M = positions,
//     y[o][h][w]        = bias[o] + sum_{dh,dw} P[(h+dh-1, w+dw-1)][(o,dh,dw)]           N = 9*Cout <= 36, K = Cin*KT)
// Every input element is an A operand exactly once per tile (read straight from global, 128-byte segments, no LDS
// staging and no tap replication); P of the tile + halo goes through LDS once and the shifted 9-term sum is the
// epilogue.  84 % of the MFMA work is useful for Cout = 3 (27 of 32 columns).
// Weights: wn[kstep][ntile][lane] = B fragment (k = (lane/32)*ksteps + kstep -> (c, dt); n = 32*ntile + lane%32 -> (o, dh, dw)).
template <int KT, int NT>
__global__ __launch_bounds__(256, 2) void conv_narrow_kernel(const ConvFwdArgs a, int ksteps, int pitch) {
  extern __shared__ __attribute__((aligned(16))) float P[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const long HW = (long)a.H * a.W;
  const int RS = a.RS;
  const int CO9 = a.Cout * 9;
  const int pt = (KT == 3 ? 1 : 0);

  const int tile = hpvg_xcd_remap(blockIdx.x, gridDim.x);
  const SkTile tc = sk_decode_tile(a, tile, 1);
  const int b = tc.b, t = tc.t, h0 = tc.q0 / RS, w0 = tc.w0;  // 2-D tiles here: L = Th * RS
  const int plload = (a.Th + 2) * RS;
  const int nblk = (plload + 31) / 32;
  const float* xb0 = a.x + (long)b * a.Cin * a.T * HW;

  // K order: half-wave h of MFMA step s holds k = h*Kh + s (Kh = ksteps), i.e. channel h*Ch + s/KT (Cin even: Ch = Cin/2)
  // and time tap s%KT: the (channel, plane) offset of a step is the same scalar for both halves and the lane part of
  // the address is a per-block constant -> scalar-base + 32-bit lane offset loads, no per-load vector address math.
  const int Kh = ksteps;
  for (int blk = wave; blk < nblk; blk += 4) {
    const int p = blk * 32 + l31;
    const int hh = p / RS, ww = p - hh * RS;
    const int gh = h0 + hh - 1, gw = w0 + ww - 1;
    const bool inimg = p < plload && gh >= 0 && gh < a.H && gw >= 0 && gw < a.W;
    const int kofs = half * Kh;                 // first k of this half-wave
    const int c_h = kofs / KT, dt_h = kofs - c_h * KT;  // (channel, time tap) of k = kofs
    // lane part of the address in bytes: (c_h, dt_h) plane + pixel (fits 32 bits: one sample is < 4 GB)
    const unsigned lofs = (unsigned)((((long)c_h * a.T + dt_h) * HW + (inimg ? gh * a.W + gw : 0)) * 4);
    const char* xbase = reinterpret_cast<const char*>(a.x + ((long)b * a.Cin * a.T + (t - pt)) * HW);
    const float* wq = a.wp + lane;
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;
    // K loop in chunks of KC steps, two register sets: the loads of chunk j+1 (inputs straight from global, weight
    // fragments from L1/L2) are in flight while the MFMAs of chunk j issue
    constexpr int KC = 16;
    float ab[2][KC], bb[2][NT][KC];
    auto load_chunk = [&](float (&av)[KC], float (&bv)[NT][KC], int s0) {
#pragma unroll
      for (int j = 0; j < KC; ++j) {
        const int s = s0 + j;                    // uniform
        const int cs = s / KT, ds = s - cs * KT; // uniform: channel / time-tap advance relative to (c_h, dt_h)
        // k = kofs + s -> (c, dt) = (c_h, dt_h) advanced by s steps of the (c, dt) odometer
        const int dtt = dt_h + ds;
        const int c = c_h + cs + (dtt >= KT ? 1 : 0);
        const int dt = dtt >= KT ? dtt - KT : dtt;
        const int tt = t + dt - pt;
        const bool ok = inimg && s < ksteps && c < a.Cin && tt >= 0 && tt < a.T;
        // byte offset of (c, dt) relative to (c_h, dt_h): ((c - c_h)*T + (dt - dt_h)) * HW * 4
        const long rel = (((long)(c - c_h) * a.T + (dt - dt_h)) * HW) * 4;
        float v = ok ? *reinterpret_cast<const float*>(xbase + rel + lofs) : 0.f;
        if (a.in_scale != nullptr && ok) {  // fused BatchNorm-apply (+ LeakyReLU) of the producer; padding stays zero
          v = v * a.in_scale[c] + a.in_shift[c];
          if (a.in_lrelu) v = hpvg_lrelu(v);
        }
        av[j] = v;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt][j] = s < ksteps ? wq[(s * NT + nt) * 64] : 0.f;
      }
    };
    auto mma_chunk = [&](const float (&av)[KC], const float (&bv)[NT][KC]) {
#pragma unroll
      for (int j = 0; j < KC; ++j)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[nt][j], acc[nt], 0, 0, 0);
    };
    load_chunk(ab[0], bb[0], 0);
    for (int s0 = 0; s0 < ksteps; s0 += 2 * KC) {
      load_chunk(ab[1], bb[1], s0 + KC);
      __builtin_amdgcn_sched_barrier(0);
      mma_chunk(ab[0], bb[0]);
      __builtin_amdgcn_sched_barrier(0);
      load_chunk(ab[0], bb[0], s0 + 2 * KC);
      __builtin_amdgcn_sched_barrier(0);
      mma_chunk(ab[1], bb[1]);
      __builtin_amdgcn_sched_barrier(0);
    }
    // C/D layout: column (n) = lane&31, row (position in the block) = (e&3) + 8*(e>>2) + 4*half
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = nt * 32 + l31;
      if (n < CO9) {
#pragma unroll
        for (int e = 0; e < 16; ++e) P[n * pitch + blk * 32 + (e & 3) + 8 * (e >> 2) + 4 * half] = acc[nt][e];
      }
    }
  }
  __syncthreads();

  // ---- epilogue: shifted 9-term sums, bias (after the accumulation), optional LeakyReLU, masked store
  const int npos = a.Th * a.Tw;
  for (int idx = tid; idx < npos; idx += 256) {
    const int hh = idx / a.Tw, ww = idx - hh * a.Tw;
    const int gh = h0 + hh, gw = w0 + ww;
    if (gh >= a.H || gw >= a.W) continue;
    const long sp = (long)t * HW + (long)gh * a.W + gw;
    for (int o = 0; o < a.Cout; ++o) {
      float v = 0.f;
#pragma unroll
      for (int dh = 0; dh < 3; ++dh)
#pragma unroll
        for (int dw = 0; dw < 3; ++dw) v += P[(o * 9 + dh * 3 + dw) * pitch + (hh + dh) * RS + ww + dw];
      if (a.bias) v += a.bias[o];
      if (a.out_lrelu) v = hpvg_lrelu(v);
      const long oi = ((long)b * a.Cout + o) * a.T * HW + sp;
      if (a.mask) v *= a.mask[oi] > 0.f ? 1.f : HPVG_LRELU_SLOPE;
      a.y[oi] = v;
    }
  }
}


// ------------------------------------------------------------------------------------------
// Narrow-output convolution, second generation (Cout <= 4, Cin even, no prologue / mask): same GEMM as conv_narrow_kernel
// (M = positions, N = (o, dh, dw), K = (c, dt); P through LDS, shifted 9-term sums as the epilogue) with the input
// streamed by 16-BYTE loads.  conv_narrow_kernel issues one dword load per lane per MFMA (vector-memory issue bound:
// 0.43 ms at stage 9 against an MFMA floor of ~0.12 ms).  Here a lane loads FOUR consecutive positions of one
// (channel, plane) with one global_load_dwordx4 and feeds them to four MFMAs as the A operand of four different
// 32-position blocks: MFMA j of a 128-position group computes the P rows of positions {128 g + 4 i + j, i = 0..31} - the
// M index of an MFMA is just a label, the P store puts every row where it belongs.  The weight fragment of a k-step is
// loaded once per four MFMAs.  For that every group of 4 positions must be contiguous in memory and inside the image:
// a tile is (Th + 2) rows x RS columns (RS % 4 == 0) of a column WINDOW that lies inside [0, W) - no halo columns are
// fetched from outside the image (band 0 starts at column 0, the last band ends at W; an output at the image border skips
// its out-of-image taps in the epilogue); rows outside the image are clamped for the load and zeroed by select.
struct Narrow2Geom {
  int RS, Th, nth, nb, npos, G, pitch;
  int ws[16], ob[16], on[16];  // per band: window start column, first output column, number of output columns
};
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte load from a 4-byte aligned address
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
template <int JB> struct AVecU;
template <> struct AVecU<4> { typedef f32x4u type; };
template <> struct AVecU<2> { typedef f32x2u type; };

template <int KT, int NT, int JB>
__global__ __launch_bounds__(256, 2) void conv_narrow2_kernel(const ConvFwdArgs a, const Narrow2Geom g, int ksteps) {
  typedef typename AVecU<JB>::type AV;
  constexpr int GP = 32 * JB;                 // positions per group (one lane: JB consecutive positions)
  constexpr int KC = KT == 3 ? 6 : 8;         // k-steps per register set (a multiple of KT: the plane of step j is j % KT)
  extern __shared__ __attribute__((aligned(16))) float P[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const long HW = (long)a.H * a.W;
  const int RS = g.RS, pitch = g.pitch;
  const int CO9 = a.Cout * 9;
  const int pt = (KT == 3 ? 1 : 0);

  // tile order: band fastest, then TIME, then the row block: consecutive workgroups (one XCD) share input planes t-1, t, t+1
  int r = hpvg_xcd_remap(blockIdx.x, gridDim.x);
  const int band = r % g.nb; r /= g.nb;
  const int t = r % a.T; r /= a.T;
  const int th = r % g.nth;
  const int b = r / g.nth;
  const int h0 = th * g.Th, wsb = g.ws[band];
  const float* xs = a.x + ((long)b * a.Cin * a.T + (t - pt)) * HW;      // plane (c = 0, dt = 0) of this tile
  const int chalf = (ksteps / KT) * half;                                // first channel of this half-wave's K range

  for (int grp = wave; grp < g.G; grp += 4) {
    const int p = GP * grp + JB * l31;
    const int pc = p < g.npos ? p : g.npos - JB;
    const int row = pc / RS, col = pc - row * RS;
    const int gh = h0 - 1 + row;
    const bool valid = p < g.npos && gh >= 0 && gh < a.H;
    const int ghc = gh < 0 ? 0 : (gh >= a.H ? a.H - 1 : gh);
    const float* lp = xs + (long)chalf * a.T * HW + (long)ghc * a.W + wsb + col;
    const float* wq = a.wp + lane;
    f32x16 acc[JB][NT];
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][nt][e] = 0.f;
    bool tok[KT];
#pragma unroll
    for (int dt = 0; dt < KT; ++dt) tok[dt] = (t + dt - pt >= 0) && (t + dt - pt < a.T);
    AV av[2][KC];
    float bv[2][KC][NT];
    auto load_chunk = [&](AV (&A)[KC], float (&Bf)[KC][NT], int s0) {
#pragma unroll
      for (int j = 0; j < KC; ++j) {
        const int s = s0 + j;
        const int dt = j % KT;                                // s0 is a multiple of KT
        const int cs = s0 / KT + j / KT;                      // channel of this step inside the half-wave's range
        if (s < ksteps && tok[dt]) {                          // uniform
          A[j] = *reinterpret_cast<const AV*>(lp + ((long)cs * a.T + dt) * HW);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) Bf[j][nt] = wq[(s * NT + nt) * 64];
        }
      }
    };
    auto mma_chunk = [&](const AV (&A)[KC], const float (&Bf)[KC][NT], int s0) {
#pragma unroll
      for (int j = 0; j < KC; ++j) {
        const int s = s0 + j;
        if (s < ksteps && tok[j % KT]) {
#pragma unroll
          for (int jj = 0; jj < JB; ++jj) {
            const float v = valid ? A[j][jj] : 0.f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[jj][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(v, Bf[j][nt], acc[jj][nt], 0, 0, 0);
          }
        }
      }
    };
    load_chunk(av[0], bv[0], 0);
    for (int s0 = 0; s0 < ksteps; s0 += 2 * KC) {
      load_chunk(av[1], bv[1], s0 + KC);
      __builtin_amdgcn_sched_barrier(0);
      mma_chunk(av[0], bv[0], s0);
      __builtin_amdgcn_sched_barrier(0);
      load_chunk(av[0], bv[0], s0 + 2 * KC);
      __builtin_amdgcn_sched_barrier(0);
      mma_chunk(av[1], bv[1], s0 + KC);
      __builtin_amdgcn_sched_barrier(0);
    }
    // C/D layout: column (n) = lane & 31, row i = (e & 3) + 8 * (e >> 2) + 4 * half; row i of MFMA jj = position GP*grp + JB*i + jj
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = nt * 32 + l31;
      if (n < CO9) {
#pragma unroll
        for (int jj = 0; jj < JB; ++jj)
#pragma unroll
          for (int e = 0; e < 16; ++e) P[n * pitch + GP * grp + JB * ((e & 3) + 8 * (e >> 2) + 4 * half) + jj] = acc[jj][nt][e];
      }
    }
  }
  __syncthreads();

  // ---- epilogue: shifted 9-term sums (taps outside the image skipped: the window holds no zero-padding columns), bias
  // after the accumulation, optional LeakyReLU
  const int ob = g.ob[band], on = g.on[band];
  const int nout = g.Th * on;
  for (int idx = tid; idx < nout; idx += 256) {
    const int hh = idx / on, cc = idx - hh * on;
    const int gh = h0 + hh, gw = ob + cc;
    if (gh >= a.H) continue;
    const long sp = (long)t * HW + (long)gh * a.W + gw;
    for (int o = 0; o < a.Cout; ++o) {
      float v = 0.f;
#pragma unroll
      for (int dh = 0; dh < 3; ++dh)
#pragma unroll
        for (int dw = 0; dw < 3; ++dw) {
          const int gwt = gw + dw - 1;
          if (gwt >= 0 && gwt < a.W) v += P[(o * 9 + dh * 3 + dw) * pitch + (hh + dh) * RS + (gwt - wsb)];
        }
      if (a.bias) v += a.bias[o];
      if (a.out_lrelu) v = hpvg_lrelu(v);
      a.y[((long)b * a.Cout + o) * a.T * HW + sp] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Narrow-output convolution with the TIME taps in N (3x3x3, Cout <= 4, Cin even, no prologue / mask).  conv_narrow2_kernel
// makes one tile per output plane with K = (c, dt): every input plane is an A operand for three output planes - three
// times the MFMAs a 64 -> 1 layer needs (9 of 32 columns used) and three fetches of every input plane.  Here one workgroup
// owns (sample, row block, column band) and walks the INPUT planes t = 0 .. T-1; per plane and output channel o
//     P[pos][(dt,dh,dw)] = sum_c x[c][t][pos] * w[o][c][dt][dh][dw]                (GEMM: M = window positions, K = Cin,
// one 32-column tile holds the 27 taps of o), P goes through LDS, and the 9-term shifted sum S_dt of slice dt is added to the
// accumulator of output plane tau = t + 1 - dt.  The three planes in flight live in registers of the thread that owns
// the position (ring rA: tau = t - 1, rB: tau = t, rC: tau = t + 1); plane tau is finished with bias and LeakyReLU and
// stored once, after input plane min(tau + 1, T - 1).  Fixed order (S_0, + S_1, + S_2, + bias), no atomics, no workspace.
// Loads as in conv_narrow2_kernel: a lane's 16-byte load of four consecutive positions feeds four MFMAs, windows lie inside
// the image, clamped rows are zeroed by select, no address outside the tensor is formed.  The weight fragments are read
// from the narrow pack as it is (wn[kstep = 3 c' + dt][ntile][lane]; this kernel's lane (half, n = (dt, j)) reads the element
// of pack column 9 o + j of k-step 3 s + dt, half-wave `half`): a few KB that stay in L1 / L2.
struct NarrowTGeom {
  int RS, Th, nth, nb, npos, G, pitch;
  int ws[16], ob[16], on[16];  // per band: window start column, first output column, number of output columns
};
constexpr int NARROWT_PPT = 4;                  // outputs per thread: Th * (widest band) <= 256 * NARROWT_PPT
constexpr size_t NARROWT_LDS_MAX = 76 * 1024;   // two workgroups per CU

template <int COUT>
__global__ __launch_bounds__(256, 2) void conv_narrowt_kernel(const ConvFwdArgs a, const NarrowTGeom g) {
  typedef f32x4u AV;
  constexpr int JB = 4, GP = 32 * JB, KC = 8, PPT = NARROWT_PPT;
  constexpr int NTO = (9 * COUT + 31) / 32;   // column tiles of the pack
  extern __shared__ __attribute__((aligned(16))) float P[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const long HW = (long)a.H * a.W;
  const int RS = g.RS, pitch = g.pitch;
  const int Ch = a.Cin >> 1;                  // k-steps: half-wave h of step s holds channel h * Ch + s

  int r = hpvg_xcd_remap(blockIdx.x, gridDim.x);
  const int band = r % g.nb; r /= g.nb;
  const int th = r % g.nth;
  const int b = r / g.nth;
  const int h0 = th * g.Th, wsb = g.ws[band], ob = g.ob[band], on = g.on[band];
  // loads: uniform base (sample, channel step, plane, window) + a 32-bit lane offset (half-wave's channel range, row, column;
  // one sample is < 4 GB) - no per-load vector address arithmetic
  const char* xb = reinterpret_cast<const char*>(a.x + (long)b * a.Cin * a.T * HW + wsb);
  const unsigned lhalf = (unsigned)((long)half * Ch * a.T * HW);
  const long cstep = a.T * HW * 4;            // bytes between channels

  // this lane's column n = l31 = (dt, j): element of the pack per output channel (columns 27 .. 31 compute nothing that is kept)
  const int dtn = l31 < 27 ? l31 / 9 : 0, j9 = l31 < 27 ? l31 - 9 * dtn : 0;
  int woff[COUT];
#pragma unroll
  for (int o = 0; o < COUT; ++o) woff[o] = (dtn * NTO + ((o * 9 + j9) >> 5)) * 64 + half * 32 + ((o * 9 + j9) & 31);
  constexpr int wstep = 3 * NTO * 64;         // floats between k-steps 3 s + dt and 3 (s + 1) + dt of the pack

  // the outputs this thread owns: idx = tid + 256 p of the band's Th x on outputs
  const int nout = g.Th * on;
  int ohh[PPT], occ[PPT];
  bool own[PPT];
  float rA[PPT][COUT], rB[PPT][COUT], rC[PPT][COUT];
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    const int idx = tid + 256 * p;
    const bool in = idx < nout;
    ohh[p] = in ? idx / on : 0;
    occ[p] = in ? idx - ohh[p] * on : 0;
    own[p] = in && h0 + ohh[p] < a.H;
#pragma unroll
    for (int o = 0; o < COUT; ++o) rA[p][o] = rB[p][o] = rC[p][o] = 0.f;
  }
  auto store_plane = [&](const float (&rr)[PPT][COUT], int tau) {
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      if (!own[p]) continue;
      const long sp = (long)tau * HW + (long)(h0 + ohh[p]) * a.W + ob + occ[p];
#pragma unroll
      for (int o = 0; o < COUT; ++o) {
        float v = rr[p][o];
        if (a.bias) v += a.bias[o];
        if (a.out_lrelu) v = hpvg_lrelu(v);
        a.y[((long)b * COUT + o) * a.T * HW + sp] = v;
      }
    }
  };

  for (int t = 0; t < a.T; ++t) {
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
      const float* wq = a.wp + woff[o];
      for (int grp = wave; grp < g.G; grp += 4) {
        const int p = GP * grp + JB * l31;
        const int pc = p < g.npos ? p : g.npos - JB;
        const int row = pc / RS, col = pc - row * RS;
        const int gh = h0 - 1 + row;
        const bool valid = p < g.npos && gh >= 0 && gh < a.H;
        const int ghc = gh < 0 ? 0 : (gh >= a.H ? a.H - 1 : gh);
        const char* xt = xb + (long)t * HW * 4;                            // uniform
        const unsigned lofs = (lhalf + (unsigned)(ghc * a.W + col)) * 4u;
        f32x16 acc[JB];
#pragma unroll
        for (int j = 0; j < JB; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
        AV av[2][KC];
        float bv[2][KC];
        auto load_chunk = [&](AV (&A)[KC], float (&Bf)[KC], int s0) {
#pragma unroll
          for (int j = 0; j < KC; ++j) {
            const int s = s0 + j;
            if (s < Ch) {                                         // uniform
              A[j] = *reinterpret_cast<const AV*>(xt + s * cstep + lofs);
              Bf[j] = wq[s * wstep];
            }
          }
        };
        auto mma_chunk = [&](const AV (&A)[KC], const float (&Bf)[KC], int s0) {
#pragma unroll
          for (int j = 0; j < KC; ++j) {
            if (s0 + j < Ch) {
#pragma unroll
              for (int jj = 0; jj < JB; ++jj)
                acc[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(valid ? A[j][jj] : 0.f, Bf[j], acc[jj], 0, 0, 0);
            }
          }
        };
        load_chunk(av[0], bv[0], 0);
        for (int s0 = 0; s0 < Ch; s0 += 2 * KC) {
          load_chunk(av[1], bv[1], s0 + KC);
          __builtin_amdgcn_sched_barrier(0);
          mma_chunk(av[0], bv[0], s0);
          __builtin_amdgcn_sched_barrier(0);
          load_chunk(av[0], bv[0], s0 + 2 * KC);
          __builtin_amdgcn_sched_barrier(0);
          mma_chunk(av[1], bv[1], s0 + KC);
          __builtin_amdgcn_sched_barrier(0);
        }
        // C/D layout: column n = lane & 31, row i = (e & 3) + 8 * (e >> 2) + 4 * half; row i of MFMA jj = position GP*grp + JB*i + jj
        if (l31 < 27) {
#pragma unroll
          for (int jj = 0; jj < JB; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) P[l31 * pitch + GP * grp + JB * ((e & 3) + 8 * (e >> 2) + 4 * half) + jj] = acc[jj][e];
        }
      }
      __syncthreads();
      // shifted 9-term sums of the three time slices (taps outside the image skipped: the window holds no padding columns)
#pragma unroll
      for (int p = 0; p < PPT; ++p) {
        if (!own[p]) continue;
        // (opaque copies: without them the 27 LDS addresses and 3 column tests of each of the thread's outputs are hoisted
        // out of the plane loop as loop invariants - ~120 registers, which spill)
        int hh = ohh[p], cc = occ[p];
        asm volatile("" : "+v"(hh), "+v"(cc));
        const int gw = ob + cc;
        const float* Pp = P + hh * RS + (gw - wsb);
        float sdt[3];
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
          float v = 0.f;
#pragma unroll
          for (int dh = 0; dh < 3; ++dh)
#pragma unroll
            for (int dw = 0; dw < 3; ++dw) {
              const int gwt = gw + dw - 1;
              if (gwt >= 0 && gwt < a.W) v += Pp[(dt * 9 + dh * 3 + dw) * pitch + dh * RS + (dw - 1)];
            }
          sdt[dt] = v;
        }
        rC[p][o] = sdt[0];
        rB[p][o] += sdt[1];
        rA[p][o] += sdt[2];
      }
      __syncthreads();
    }
    if (t >= 1) store_plane(rA, t - 1);      // its last contribution (slice 2 of plane t) is in
#pragma unroll
    for (int p = 0; p < PPT; ++p)
#pragma unroll
      for (int o = 0; o < COUT; ++o) { rA[p][o] = rB[p][o]; rB[p][o] = rC[p][o]; }
  }
  store_plane(rA, a.T - 1);                  // no plane T: the last output plane is complete after plane T - 1
}

// B fragments of the narrow kernel; transpose_flip as in conv_pack_kernel
__global__ void conv_pack_narrow_kernel(const float* __restrict__ w, const float* __restrict__ inv_scale, float* __restrict__ wn,
                                        int Cin_k, int Cout_k, int KT, int NT, int ksteps, int transpose_flip, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int lane = idx & 63;
  long r = idx >> 6;
  const int nt = r % NT;
  const int s = (int)(r / NT);
  const int k = (lane >> 5) * ksteps + s;  // half-wave h holds k = h*ksteps + s (see conv_narrow_kernel)
  const int n = nt * 32 + (lane & 31);
  const int c = k / KT, dt = k - c * KT;
  const int o = n / 9, tap = dt * 9 + (n - o * 9);
  const int taps = KT * 9;
  float val = 0.f;
  if (o < Cout_k && c < Cin_k) {
    if (!transpose_flip) val = w[((long)o * Cin_k + c) * taps + tap];
    else val = w[((long)c * Cout_k + o) * taps + (taps - 1 - tap)];
    if (inv_scale) val *= inv_scale[0];
  }
  wn[idx] = val;
}

// ------------------------------------------------------------------------------------------
// weight pack: natural [Cout][Cin][taps] -> MFMA A-fragment order
//   wp[chunk][tap][mblock][lane][cp] = Wsrc[o = mblock*32 + (lane&31)][c = chunk*CC + 2cp + (lane>>5)][tap]
// transpose_flip=1 packs the backward-data weights (Wsrc[o'][c'][tap] = W[c'][o'][ntaps-1-tap]).
// A device scalar `inv_scale` (1/sigma of spectral norm) is folded in when given.
// Behind the direct pack (`total_direct` floats) follow the Winograd U fragments of the same weight when the layer is wide
// enough for conv_wino_kernel (conv_wino.inl); which of the two a launch reads is decided per shape in conv_fwd_impl.
__global__ void conv_pack_kernel(const float* __restrict__ w, const float* __restrict__ inv_scale, float* __restrict__ wp,
                                 int Cin_k, int Cout_k, int taps, int CC, int nchunk, int mbtot, int transpose_flip,
                                 long total_direct, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  if (idx >= total_direct) {
    const long iw = idx - total_direct;
    const long nw1 = ((long)((Cin_k + WINO_CC - 1) / WINO_CC) * (taps / 9) * 3 * 4 + 4) * mbtot * 64 * (WINO_CC / 2);   // wino_pack_floats
    float val = iw < nw1 ? wino_pack_value(w, iw, Cin_k, Cout_k, taps / 9, (Cin_k + WINO_CC - 1) / WINO_CC, mbtot, transpose_flip)
                         : wino2_pack_value(w, iw - nw1, Cin_k, Cout_k, (Cin_k + 3) / 4, 2 * ((mbtot + 1) / 2), transpose_flip);
    if (inv_scale) val *= inv_scale[0];
    wp[idx] = val;
    return;
  }
  const int CP = CC / 2;
  long r = idx;
  const int cp = r % CP; r /= CP;
  const int lane = r % 64; r /= 64;
  const int mb = r % mbtot; r /= mbtot;
  const int tap = r % taps; r /= taps;
  const int ch = (int)r;
  float val = 0.f;
  if (ch < nchunk) {  // else: tail padding stays zero
    const int o = mb * 32 + (lane & 31);
    const int c = ch * CC + 2 * cp + (lane >> 5);
    if (o < Cout_k && c < Cin_k) {
      if (!transpose_flip) val = w[((long)o * Cin_k + c) * taps + tap];
      else val = w[((long)c * Cout_k + o) * taps + (taps - 1 - tap)];
      if (inv_scale) val *= inv_scale[0];
    }
  }
  wp[idx] = val;
}

// the same for up to HPVG_PACK_BATCH_MAX weights of ONE layer shape in a single launch (blockIdx.y = item); flip per item
struct PackBatchArgs {
  const float* w[HPVG_PACK_BATCH_MAX];
  float* wp[HPVG_PACK_BATCH_MAX];
  int flip[HPVG_PACK_BATCH_MAX];
};
__global__ void conv_pack_batch_kernel(const PackBatchArgs a, int C, int taps, int CC, int nchunk, int mbtot, long total_direct,
                                       long total) {
  // square layers only (Cin == Cout == C): the forward and the flipped pack then share every size
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int it = blockIdx.y;
  const float* __restrict__ w = a.w[it];
  const int transpose_flip = a.flip[it];
  if (idx >= total_direct) {
    const long iw = idx - total_direct;
    const long nw1 = ((long)((C + WINO_CC - 1) / WINO_CC) * (taps / 9) * 3 * 4 + 4) * mbtot * 64 * (WINO_CC / 2);   // wino_pack_floats
    a.wp[it][idx] = iw < nw1 ? wino_pack_value(w, iw, C, C, taps / 9, (C + WINO_CC - 1) / WINO_CC, mbtot, transpose_flip)
                             : wino2_pack_value(w, iw - nw1, C, C, (C + 3) / 4, 2 * ((mbtot + 1) / 2), transpose_flip);
    return;
  }
  const int CP = CC / 2;
  long r = idx;
  const int cp = r % CP; r /= CP;
  const int lane = r % 64; r /= 64;
  const int mb = r % mbtot; r /= mbtot;
  const int tap = r % taps; r /= taps;
  const int ch = (int)r;
  float val = 0.f;
  if (ch < nchunk) {
    const int o = mb * 32 + (lane & 31);
    const int c = ch * CC + 2 * cp + (lane >> 5);
    if (o < C && c < C) {
      if (!transpose_flip) val = w[((long)o * C + c) * taps + tap];
      else val = w[((long)c * C + o) * taps + (taps - 1 - tap)];
    }
  }
  a.wp[it][idx] = val;
}

// ================================================================================================================ host part
// Knobs, planners, plan memo, scratch, the decision, launches, entry points - the layout of conv_wgrad.hip.
struct CShape { int B, Cin, Cout, T, H, W, KT; };   // kernel view of one launch (2-D: T = 1, KT = 1)
// HPVG_ERR_ARG for a dimension below 1, HPVG_ERR_UNSUPPORTED for a kernel depth other than 1 or 3
inline int conv_check(const CShape& c) {
  if (c.B < 1 || c.Cin < 1 || c.Cout < 1 || c.T < 1 || c.H < 1 || c.W < 1) return HPVG_ERR_ARG;
  return c.KT == 1 || c.KT == 3 ? HPVG_OK : HPVG_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------------------------ knobs
// Every knob of the forward host path, read from the environment once, on first use.  The fields below the line are what
// is in force: hpvg_conv_wino_config rewrites them at run time (tests and A/B tools).
struct CKnobs {
  bool sk_off;         // HPVG_CONV_SK=0: the one-workgroup-per-tile schedule even with a workspace
  bool narrow2_off;    // HPVG_NARROW2=0: the first-generation narrow kernel for every tail
  int narrowt;         // HPVG_NARROWT (in force; hpvg_conv_narrowt_config rewrites it): conv_narrowt_kernel 0 = by size, 1 = never,
                       // 2 = wherever it can run
  // HPVG_WINO2R=0 keeps the first-generation two-axis kernel (every wave all 16 points of one block: conv_wino2d_kernel);
  // default: the points split over the waves by row (conv_wino2r_kernel: half the input-transform instructions and U loads
  // per MFMA)
  bool w2r;
  bool w2d_off;        // HPVG_WINO2D=0: no two-axis section in the packs, no two-axis kernel in the dispatch
  bool w2_split_off;   // HPVG_W2_SPLIT=0: conv_wino2r_kernel in whole-tile rounds only (w2_split_plan)
  int stagger;         // HPVG_WINO_STAGGER: ConvFwdArgs::stagger of a one-axis launch with two workgroups per CU
  int only_nb, only_mb, only_ntw;   // development: HPVG_PLAN_NB / _MB / _NTW restrict the wide searches to one value
  // HPVG_WINO as the process started: 0 = no Winograd path at all (the weight packs carry no U fragments either, and
  // hpvg_conv_wino_config refuses), 2 = every eligible launch, 1 / unset = eligible launches of at least min_pos positions
  int env_wino;
  // ---- in force
  int wino;            // 0 = direct kernel only, 2 = every eligible launch, else by size
  long min_pos;        // HPVG_WINO_MIN: the one-axis threshold in output positions B*T*H*W (< 0: conv_use_wino's defaults)
  int stg;             // HPVG_WINO_STG, conv_wino_kernel's staging form: 0 = by size, 1 = halo'd bands only, 2 = rows as in memory wherever it fits
  int w2d;             // the two-axis kernel: 0 = by size, 1 = never, 2 = wherever it can run
  int gen;             // bumped when stg changes: what plan_wino_search may pick has changed, the plan memo drops its entries
};
CKnobs& cknobs() {
  static CKnobs knobs = [] {
    auto num = [](const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; };
    CKnobs k{};
    k.sk_off = num("HPVG_CONV_SK", 1) == 0;
    k.narrow2_off = num("HPVG_NARROW2", 1) == 0;
    const long nt = num("HPVG_NARROWT", 0);
    k.narrowt = nt == 1 || nt == 2 ? (int)nt : 0;
    k.w2r = num("HPVG_WINO2R", 1) != 0;
    k.w2d_off = num("HPVG_WINO2D", 1) == 0;
    k.w2_split_off = num("HPVG_W2_SPLIT", 1) == 0;
    k.stagger = (int)num("HPVG_WINO_STAGGER", 0);
    k.only_nb = (int)num("HPVG_PLAN_NB", 0);
    k.only_mb = (int)num("HPVG_PLAN_MB", 0);
    k.only_ntw = (int)num("HPVG_PLAN_NTW", 0);
    k.wino = k.env_wino = (int)num("HPVG_WINO", 1);
    k.min_pos = num("HPVG_WINO_MIN", -1);
    const long stg = num("HPVG_WINO_STG", 0);
    k.stg = stg == 1 || stg == 2 ? (int)stg : 0;
    return k;
  }();
  return knobs;
}

// which layers have which kernels (and pack sections)
inline int conv_cc(int Cin) { return Cin <= 4 ? 4 : 8; }
inline bool conv_is_narrow(int Cin, int Cout) { return Cout <= 4 && Cin > 4; }
inline bool conv_is_wino(const CKnobs& k, int Cin, int Cout) { return k.env_wino != 0 && Cin >= 8 && Cout > 32; }
// the two-axis kernel (conv_wino2d.inl) has its own fragment section behind the one-axis one for the 3x3x3 layers
inline bool conv_is_wino2d(const CKnobs& k, int Cin, int Cout, int KT) { return !k.w2d_off && KT == 3 && conv_is_wino(k, Cin, Cout); }

// floats of the direct kernel's A-fragment pack (the Winograd fragments, when the layer has them, follow it)
inline size_t direct_pack_floats(int Cin, int Cout, int KT) {
  const int CC = conv_cc(Cin);
  const int nchunk = hpvg_cdiv(Cin, CC);
  const int mbtot = hpvg_cdiv(Cout, 32);
  const size_t per_tap = (size_t)mbtot * 64 * (CC / 2);
  return ((size_t)nchunk * KT * 9 + 2) * per_tap;  // +2 taps of zero tail padding (A prefetch runs one tap / one m-tile ahead)
}
// number of floats of the packed-weight buffer for a conv with Cin -> Cout (kernel view)
size_t wpack_floats(int Cin, int Cout, int KT, bool with2d) {
  const CKnobs& k = cknobs();
  if (conv_is_narrow(Cin, Cout)) return (size_t)hpvg_cdiv(Cin * KT, 2) * hpvg_cdiv(9 * Cout, 32) * 64;  // wn[kstep][ntile][lane]
  return direct_pack_floats(Cin, Cout, KT) + (conv_is_wino(k, Cin, Cout) ? wino_pack_floats(Cin, Cout, KT) : 0) +
         (with2d && conv_is_wino2d(k, Cin, Cout, KT) ? wino2_pack_floats(Cin, Cout) : 0);
}

// ---------------------------------------------------------------------------------------------------------------- planners
struct Plan {
  int Th, Tw, RS, PL, L, qstride, nrange, ntw, nblocks, NB, MB, gridy, nj;  // Th != 0 only for the narrow kernel's 2-D tiles
  size_t lds;  // bytes of the LDS tile buffer
  int stg;     // conv_wino_kernel: 2 = rows-as-in-memory staging with 16-byte pieces (conv_wino.inl), else the halo'd bands
};

constexpr long CONV_SLOTS = 2L * HPVG_NUM_CU;  // co-resident workgroups: two per CU (256 VGPRs each, LDS <= 80 KB)
inline long conv_slots(int MB, int NB) { return (long)HPVG_CONV_WGS(MB, NB) * HPVG_NUM_CU; }

// Cost in us of one wide launch of ntl tiles of nchunk items each, for both wide planners.  streamk = true: the launch is
// S = min(items, slots) persistent workgroups that share the (tile, chunk) items evenly (needs the partial-slab workspace).
// streamk = false: one workgroup per tile, dealt out by the hardware dispatcher (no workspace; grids of 1-5 tiles per slot
// are quantised - the reason stream-K exists): whole tiles per CU, pairs run together, an odd one runs alone at the end.
// Constants chosen to minimise the REGRET of the plan picked over the measured landscapes of stages 3-9 at B = 2 and 4
// (tools/ab_conv_plan.sh: every band count x NB forced; mean regret 0.3 %, worst 1.6 %; tools/perf_conv.py, stages 5-9,
// within 5 %): an item costs its MFMA rounds (mfma_paired when two workgroups share the CU's matrix pipe, mfma_alone
// otherwise) + ~6 us of staging / barrier work the co-resident workgroup does not hide (2 when alone) + the input planes it
// stages (stage_us); tiles cut across workgroups travel through HBM as raw accumulator slabs (16 KB per 32x32 block, `blocks`
// of them, written by the main kernel, read back by the fix-up: ~5.5 us per block at the chip's share of bandwidth).
// The planners break ties at 1e-9: keep the order of the operations (`blocks` is a power of two).
inline double conv_cost(bool streamk, long ntl, int nchunk, long slots, double mfma_paired, double mfma_alone, double stage_us,
                        int blocks) {
  if (!streamk) {
    const long per_cu = (ntl + HPVG_NUM_CU - 1) / HPVG_NUM_CU;
    const double tile_paired = nchunk * (mfma_paired + 6.0 + stage_us) + 0.4 * blocks;
    const double tile_alone = nchunk * (mfma_alone + 2.0 + stage_us) + 0.4 * blocks;
    return (double)(per_cu / 2) * tile_paired + (double)(per_cu & 1) * tile_alone + 1e-4 * (double)ntl;
  }
  const long items_tot = ntl * nchunk;
  const long S = items_tot < slots ? items_tot : slots;
  const long ndp = ntl / S;
  const long rem = (ntl - ndp * S) * nchunk;
  const double items = (double)(ndp * nchunk) + (double)((rem + S - 1) / S);
  const bool paired = S > HPVG_NUM_CU;
  const double per_item = (paired ? mfma_paired : mfma_alone) + (paired ? 6.0 : 2.0) + stage_us;
  const double tiles = (double)(ndp + (rem ? 1 : 0));
  double parts = 0.0;
  if (rem) {
    parts = 1.0 + (double)rem / (double)S / (double)nchunk;
    if (parts > 2.0) parts = 2.0;
  }
  return items * per_item + tiles * 0.4 * blocks + parts * 5.5 * blocks + 1e-4 * (double)ntl;
}

// 2-D tiles (Th x Tw) for conv_narrow_kernel: a GEMM over the tile + halo positions, one workgroup per tile: blocks of 32
// positions over 4 waves, K steps of 64 cycles each, ~3 us of epilogue; the P image (9*Cout rows) must leave room for >= 4
// workgroups per CU (they hide the load latency)
Plan plan_narrow_search(const CShape& c) {
  const auto [B, Cin, Cout, T, H, W, KT] = c;
  Plan best{};
  double best_cost = 1e300;
  for (int Tw = 1; Tw <= W; ++Tw) {
    const int ntw = hpvg_cdiv(W, Tw);
    if (Tw != hpvg_cdiv(W, ntw)) continue;  // only balanced splits of W
    const int RS = Tw + 2;
    for (int Th = 1; Th <= H; ++Th) {
      const int nth = hpvg_cdiv(H, Th);
      if (Th != hpvg_cdiv(H, nth)) continue;
      const int nblk_h = hpvg_cdiv((Th + 2) * RS, 32);
      if ((Th + 2) * RS > NJMAX * 256) break;
      if ((size_t)(9 * Cout) * ((size_t)nblk_h * 32 + 1) * sizeof(float) > 38 * 1024) continue;
      const long ntl = (long)B * T * nth * ntw;
      const double per_tile = hpvg_cdiv(nblk_h, 4) * (double)hpvg_cdiv(Cin * KT, 2) * hpvg_cdiv(9 * Cout, 32) * 0.033 + 3.0;
      const double waves = ntl <= CONV_SLOTS ? 1.0 : (double)ntl / (double)CONV_SLOTS;
      const double cost = waves * per_tile + 1e-3 * (double)ntl;
      if (cost < best_cost - 1e-9) {
        best_cost = cost;
        best = Plan{Th, Tw, RS, (Th + 2) * RS, Th * RS, Th * RS, nth, ntw, hpvg_cdiv(Th * RS, 32), 4, 1, 1, hpvg_cdiv((Th + 2) * RS, 256), 0};
      }
    }
  }
  return best;
}

// conv_mfma_kernel: W is cut into ntw balanced bands of Tw columns; a band plane, flattened row by row with stride RS = Tw+2
// (its two halo columns are the junk GEMM columns), is cut into nrange balanced ranges of L <= NB*128 positions.  Wide
// bands waste few junk columns, and a range - unlike a whole number of rows - fills its 32-position blocks.  An MFMA round
// (32 positions x 32 channels x 8-channel chunk) costs 6.5 us paired, 3.0 alone; staging 2 us per 1000 positions.
Plan plan_conv_search(const CKnobs& k, const CShape& c, bool streamk) {
  const auto [B, Cin, Cout, T, H, W, KT] = c;
  const int CC = conv_cc(Cin);
  const int nchunk = hpvg_cdiv(Cin, CC);
  const int mbtot = hpvg_cdiv(Cout, 32);
  Plan best{};
  double best_cost = 1e300;
  for (int MB = (mbtot >= 2 ? 2 : 1); MB >= 1; --MB) {
    if (k.only_mb && MB != k.only_mb && mbtot >= 2) continue;
    const int gridy = hpvg_cdiv(mbtot, MB);
    for (int ntw = 1; ntw <= W; ++ntw) {
      const int Tw = hpvg_cdiv(W, ntw);
      if (ntw > 1 && hpvg_cdiv(W, ntw - 1) == Tw) continue;  // same band width as the previous ntw: more bands, no gain
      if (k.only_ntw && ntw != k.only_ntw) continue;
      const int RS = Tw + 2;
      const long flat = (long)(H - 1) * RS + Tw;  // flattened positions that hold outputs
      // candidate tiles of this band.  3x3x3: balanced ranges of at most NB*128 positions.  3x3 (a third of the MFMA work
      // per staged plane, so the cost constants fitted on 3x3x3 launches do not rank these well): whole rows only, the
      // tile family the 2-D path was tuned and measured with.
      const int ncand = KT == 3 ? 3 : H;
      for (int cand = 0; cand < ncand; ++cand) {
        int NB, L, nrange, qstride;
        if (KT == 3) {
          NB = 1 << cand;
          nrange = hpvg_cdiv(flat, NB * 128);
          L = hpvg_cdiv(flat, nrange);
          qstride = L;
        } else {
          const int Th = cand + 1;
          nrange = hpvg_cdiv(H, Th);
          if (Th != hpvg_cdiv(H, nrange)) continue;  // only balanced splits of H
          L = Th * RS;
          const int nblk = (L - 3) / 32 + 1;          // last output position of the tile: (Th-1)*RS + Tw - 1
          if (nblk > 16) break;
          const int rounds = hpvg_cdiv(nblk, 4);
          NB = rounds <= 1 ? 1 : (rounds == 2 ? 2 : 4);
          qstride = L;
          if (L > NB * 128) L = NB * 128;             // the (at most two) positions cut off are halo columns
        }
        if (k.only_nb && NB != k.only_nb) continue;
        const int Lmax = NB * 128;
        const int plload = L + 2 * RS + 2;
        if (plload > NJMAX * 256) continue;
        const int PL = Lmax + 2 * RS + 2;  // lanes past L still read (junk) operands inside the buffer
        const size_t lds = (size_t)CC * KT * PL * sizeof(float);
        if (lds > (HPVG_CONV_WGS(MB, NB) == 4 ? 38 : 80) * 1024) continue;
        const long ntl = (long)B * T * nrange * ntw * gridy;
        const double cost = conv_cost(streamk, ntl, nchunk, conv_slots(MB, NB), (double)NB * MB * 6.5, (double)NB * MB * 3.0,
                                      0.002 * plload, NB * MB);
        if (cost < best_cost - 1e-9) {
          best_cost = cost;
          best = Plan{0, Tw, RS, PL, L, qstride, nrange, ntw, hpvg_cdiv(L, 32), NB, MB, gridy, hpvg_cdiv(plload, 256), lds};
        }
      }
    }
  }
  return best;
}

// Tile plan of conv_wino_kernel: bands of an EVEN width Tw (row stride RS = Tw + 2 even: an output pair never straddles a
// row), a band plane cut into balanced ranges of an even L <= NBP*128 positions (NBP*64 pairs).  Same cost form as above
// with the Winograd item: 36 instead of 27 MFMA k-steps per channel pair on half the positions per accumulator set.
Plan plan_wino_search(const CKnobs& k, const CShape& c, bool streamk) {
  const auto [B, Cin, Cout, T, H, W, KT] = c;
  const int nchunk = hpvg_cdiv(Cin, WINO_CC);
  const int mbtot = hpvg_cdiv(Cout, 32);
  const int gridy = hpvg_cdiv(mbtot, 2);
  Plan best{};
  double best_cost = 1e300;
  const int Lmax = WINO_NBP * 128;
  if (k.stg != 1 && (W & 1) == 0 && W >= 2) {
    // staging form 2: one band of the full width, row stride W, no halo columns, a quarter of the staging instructions.
    // Measured (profiles/r02_perf_wino_stg2.txt): -4.2 % at stage 9, -3.7 % at stage 8, +-1-2 % at stages 5-7, where a
    // workgroup sees fewer than two whole tiles: taken from two tiles per co-resident workgroup up (or when forced).
    const long flat = (long)H * W;
    const int nrange = hpvg_cdiv(flat, Lmax);
    int L = hpvg_cdiv(flat, nrange);
    L += L & 1;
    // The image sits one float into its plane slot and is WRITTEN in whole 16-byte groups: up to (2 W + Lmax + 8) / 4 of
    // them, so the slot holds 1 + 2 W + Lmax + 8 floats, rounded up to an even count (reads reach sh + 2 * (Lmax/2 - 1) +
    // 2 * W + 3 <= 2 W + Lmax + 5 only).  With 2 W + Lmax + 8 floats the last group of the last plane ended one float past
    // the workgroup's LDS, and where the allocation is a whole number of LDS granules (24 planes x 680 floats at W = 208,
    // x 800 at W = 268) the hardware dropped that whole group: the last pair of every tile read a stale d3 for one channel
    // of each chunk.
    const int PL = 2 * W + Lmax + 10;
    const size_t lds = (size_t)WINO_CC * KT * PL * sizeof(float);
    const int ngmax = (L + 2 * W + 2 + 3 + 3) >> 2;           // 16-byte groups of the staged span: one per lane
    const long ntl = (long)B * T * nrange * gridy;
    if (lds <= 80 * 1024 && ngmax <= 256 && (k.stg == 2 || ntl >= 2 * CONV_SLOTS))
      return Plan{0, W, W, PL, L, L, nrange, 1, hpvg_cdiv(L, 32), WINO_NBP, 2, gridy, 1, lds, 2};
  }
  int prev_tw = 0;
  for (int ntw = 1; ntw <= W; ++ntw) {
    int Tw = hpvg_cdiv(W, ntw);
    Tw += Tw & 1;
    if (Tw == prev_tw || (long)(ntw - 1) * Tw >= W) continue;  // same band width as before / an empty last band
    prev_tw = Tw;
    if (k.only_ntw && ntw != k.only_ntw) continue;
    const int RS = Tw + 2;
    const long flat = (long)(H - 1) * RS + Tw;
    const int nrange = hpvg_cdiv(flat, Lmax);
    int L = hpvg_cdiv(flat, nrange);
    L += L & 1;
    const int plload = L + 2 * RS + 2;
    if (plload > NJMAX * 256) continue;
    const int PL = Lmax + 2 * RS + 2;   // even; lanes past L still read (junk) operands inside the buffer
    const size_t lds = (size_t)WINO_CC * KT * PL * sizeof(float);
    if (lds > 80 * 1024) continue;
    const long ntl = (long)B * T * nrange * ntw * gridy;
    // (staging weighs half of what it does for the direct kernel: measured landscape, profiles/r02_ab_wino_plan.txt - wide
    // bands with few junk columns win at stages 7-9 although they stage three rows per row of outputs)
    const double mfma_paired = 6.5 * (2.0 * WINO_NBP) * (2.0 / 3.0);  // 64 ch x NBP*64 pairs = 2*NBP direct 32x32 block pairs, at 36/54 of their k-steps
    const double cost = conv_cost(streamk, ntl, nchunk, CONV_SLOTS, mfma_paired, mfma_paired * 3.0 / 6.5, 0.001 * plload, 2 * WINO_NBP);
    if (cost < best_cost - 1e-9) {
      best_cost = cost;
      best = Plan{0, Tw, RS, PL, L, L, nrange, ntw, hpvg_cdiv(L, 32), WINO_NBP, 2, gridy, hpvg_cdiv(plload, 256), lds};
    }
  }
  return best;
}

// Geometry of the two-axis Winograd kernels (conv_wino2d.inl, conv_wino2r.inl); ok = false where they cannot run
struct W2Geom {
  int Cq, R, ntq, tqw, gridy, nsc, ntl;
  int sp_full, sp_parts, sp_wgs;   // w2_split_plan: tiles of the whole-tile launch, parts per leftover tile (1: no split), workgroups of the part launch
  bool ok;
};
// conv_wino2r_kernel runs whole tiles, one persistent workgroup per CU: ceil(ntl / 256) rounds, the last one as long as the
// others however few tiles it holds (6 of 256 at level 6, B = 2).  A thinly filled last round is cut out of the whole-tile
// launch and run by a second launch of the kernel's SUB instances, one PART of a tile per workgroup - no workspace, no
// partial sums, the same bits (conv_wino2r.inl): with r = ntl mod 256 leftover tiles after at least one full round,
// r <= 64: 4 r quarter tiles (one 32 x 32 block each), r <= 128: 2 r half tiles (one quad half each); the parts fit one
// round.  More leftover tiles, a launch of one round or less, the first-generation kernel, HPVG_W2_SPLIT=0: whole tiles.
void w2_split_plan(const CKnobs& k, W2Geom& q) {
  q.sp_full = q.ntl; q.sp_parts = 1; q.sp_wgs = 0;
  const int r = q.ntl % HPVG_NUM_CU;
  if (k.w2_split_off || !k.w2r || q.ntl <= HPVG_NUM_CU || r == 0 || r > HPVG_NUM_CU / 2) return;
  q.sp_parts = r <= HPVG_NUM_CU / 4 ? 4 : 2;
  q.sp_full = q.ntl - r;
  q.sp_wgs = r * q.sp_parts;
}
W2Geom wino2d_geom(const CKnobs& k, const CShape& c) {
  const auto [B, Cin, Cout, T, H, W, KT] = c;
  W2Geom q{};
  if (!conv_is_wino2d(k, Cin, Cout, KT) || ((W & 1) && !k.w2r) || W < 2 || (long)H * W < 4) return q;   // (odd W: conv_wino2r_kernel's ODD instance)
  if (k.w2r && (long)H * W + 4 > HPVG_ZERO_PLANE_FLOATS) return q;                                       // (its zero plane)
  q.Cq = (W + 1) / 2;
  q.R = hpvg_cdiv(H, 2);
  const int nq = q.R * q.Cq;
  q.ntq = hpvg_cdiv(nq, 64);                            // tiles per plane: 64 consecutive quads each
  q.tqw = 64;
  // the staged span of every tile (first input of its first quad, rounded down to a multiple of 4, to the last input of its
  // last quad): one 16-byte group per lane
  for (int tp = 0; tp < q.ntq; ++tp) {
    const int Q0 = tp * 64, R0 = Q0 / q.Cq, c0 = Q0 - R0 * q.Cq;
    int Ql = Q0 + 63;
    if (Ql > nq - 1) Ql = nq - 1;
    const int R1 = Ql / q.Cq, c1 = Ql - R1 * q.Cq;
    const int lo = (2 * R0 - 1) * W + 2 * c0 - 1;
    const int lo4 = lo >= 0 ? (lo & ~3) : -((3 - lo) & ~3);
    const int hi = (2 * R1 + 2) * W + 2 * c1 + 3;
    if (hi - lo4 > 1024) return q;
  }
  q.gridy = hpvg_cdiv(hpvg_cdiv(Cout, 32), 2);
  q.nsc = hpvg_cdiv(Cin, 4);
  const long ntl = (long)B * T * q.ntq * q.gridy;
  if (ntl > 0x7fffffffL) return q;
  q.ntl = (int)ntl;
  w2_split_plan(k, q);
  q.ok = true;
  return q;
}

// tile plan of conv_narrow2_kernel; returns false when the shape does not fit (then conv_narrow_kernel runs)
bool plan_narrow2(int B, int Cin, int Cout, int T, int H, int W, int KT, Narrow2Geom* out, long* ntiles) {
  if ((Cin & 1) || W < 4) return false;
  const int NT = hpvg_cdiv(9 * Cout, 32);
  const int JB = NT == 1 ? 4 : 2;
  const int GP = 32 * JB;
  double best = 1e300;
  bool found = false;
  // bands of a window width RS: band 0 = window [0, RS), outputs columns 0 .. RS-2 (all W of them when RS == W); a middle
  // band outputs RS-2 columns from the window that starts one column before its first output; a band whose remaining
  // columns number <= RS-1 is the last: its window is pulled back to end at W (the right image border needs no neighbour)
  auto bands = [&](int RS, Narrow2Geom* q) -> int {
    int nb = 0, o = 0;
    while (o < W) {
      if (nb == 16) return 0;
      int n, ws;
      if (nb == 0) { n = (RS == W) ? W : RS - 1; ws = 0; }
      else if (W - o <= RS - 1) { n = W - o; ws = W - RS; }
      else { n = RS - 2; ws = o - 1; }
      if (n < 1) return 0;
      if (q) { q->ws[nb] = ws; q->ob[nb] = o; q->on[nb] = n; }
      o += n;
      ++nb;
    }
    return nb;
  };
  for (int RS = 4; RS <= 256 && RS <= W; RS += 4) {
    const int nb = bands(RS, nullptr);
    if (nb == 0) continue;
    for (int Th = 1; Th <= H; ++Th) {
      const int nth = hpvg_cdiv(H, Th);
      if (Th != hpvg_cdiv(H, nth)) continue;
      const int npos = (Th + 2) * RS;
      const int G = hpvg_cdiv(npos, GP);
      if (G > 16) break;
      const int pitch = (G * GP) | 1;
      if ((size_t)(9 * Cout) * pitch * sizeof(float) > 76 * 1024) break;
      const long nt = (long)B * T * nth * nb;
      const double rounds = hpvg_cdiv(G, 4);
      const double waves = nt <= 2L * HPVG_NUM_CU ? 1.0 : (double)nt / (2.0 * HPVG_NUM_CU);
      const double cost = waves * (rounds * GP + 30.0);     // MFMA work of the slowest wave + a fixed per-tile cost (epilogue, barrier)
      if (cost < best) {
        best = cost;
        found = true;
        Narrow2Geom q{};
        q.RS = RS; q.Th = Th; q.nth = nth; q.nb = nb; q.npos = npos; q.G = G; q.pitch = pitch;
        bands(RS, &q);
        *out = q;
        *ntiles = nt;
      }
    }
  }
  if (!found) return false;
  // every output column needs its in-image neighbours inside the band's window
  for (int k = 0; k < out->nb; ++k) {
    const int lo = out->ob[k] - 1 < 0 ? 0 : out->ob[k] - 1;
    const int hi = out->ob[k] + out->on[k] > W - 1 ? W - 1 : out->ob[k] + out->on[k];
    if (out->on[k] < 0 || lo < out->ws[k] || hi >= out->ws[k] + out->RS) return false;
  }
  return true;
}

// tile plan of conv_narrowt_kernel; returns false when the shape cannot run on it.  A tile is (Th + 2) rows x RS columns of a
// column window inside [0, W), the bands as in plan_narrow2; P holds 27 columns whatever Cout is, and a thread owns at most
// NARROWT_PPT outputs of a band.  A workgroup is matrix-core bound and walks all T planes, so the launch takes as long as the
// busiest CU: ceil(workgroups / CUs) workgroups of Cout * (MFMA rounds of the slowest wave + a fixed epilogue) per plane.
bool plan_narrowt(int B, int Cin, int Cout, int T, int H, int W, int KT, NarrowTGeom* out, long* nwg) {
  if (KT != 3 || (Cin & 1) || Cin < 2 || Cout > 4 || W < 4) return false;
  if ((long)Cin * T * H * W >= (1L << 30)) return false;   // the kernel's 32-bit lane offsets span one sample
  constexpr int GP = 128;
  double best = 1e300;
  bool found = false;
  auto bands = [&](int RS, NarrowTGeom* q) -> int {
    int nb = 0, o = 0;
    while (o < W) {
      if (nb == 16) return 0;
      int n, ws;
      if (nb == 0) { n = (RS == W) ? W : RS - 1; ws = 0; }
      else if (W - o <= RS - 1) { n = W - o; ws = W - RS; }
      else { n = RS - 2; ws = o - 1; }
      if (n < 1) return 0;
      if (q) { q->ws[nb] = ws; q->ob[nb] = o; q->on[nb] = n; }
      o += n;
      ++nb;
    }
    return nb;
  };
  for (int RS = 4; RS <= 256 && RS <= W; RS += 4) {
    const int nb = bands(RS, nullptr);
    if (nb == 0) continue;
    const int on_max = RS == W ? W : RS - 1;
    for (int Th = 1; Th <= H; ++Th) {
      const int nth = hpvg_cdiv(H, Th);
      if (Th != hpvg_cdiv(H, nth)) continue;
      if (Th * on_max > 256 * NARROWT_PPT) break;
      const int npos = (Th + 2) * RS;
      const int G = hpvg_cdiv(npos, GP);
      const int pitch = (G * GP) | 1;
      if ((size_t)27 * pitch * sizeof(float) > NARROWT_LDS_MAX) break;
      const long n = (long)B * nth * nb;
      // (ties - small levels, where one workgroup per CU is never reached - go to the least total work: the least halo)
      const double cost = (double)hpvg_cdiv(n, (long)HPVG_NUM_CU) * (hpvg_cdiv(G, 4) * GP + 40.0) + 1e-3 * (double)(n * G);
      if (cost < best) {
        best = cost;
        found = true;
        NarrowTGeom q{};
        q.RS = RS; q.Th = Th; q.nth = nth; q.nb = nb; q.npos = npos; q.G = G; q.pitch = pitch;
        bands(RS, &q);
        *out = q;
        *nwg = n;
      }
    }
  }
  if (!found) return false;
  // every output column needs its in-image neighbours inside the band's window, and every window lies inside the image
  for (int k = 0; k < out->nb; ++k) {
    const int lo = out->ob[k] - 1 < 0 ? 0 : out->ob[k] - 1;
    const int hi = out->ob[k] + out->on[k] > W - 1 ? W - 1 : out->ob[k] + out->on[k];
    if (out->on[k] < 1 || lo < out->ws[k] || hi >= out->ws[k] + out->RS) return false;
    if (out->ws[k] < 0 || out->ws[k] + out->RS > W) return false;
  }
  return true;
}
inline size_t narrowt_lds(const NarrowTGeom& g) { return (size_t)27 * g.pitch * sizeof(float); }
// Where conv_narrowt_kernel is taken, by size where it was measured to win against conv_narrow2_kernel (DESIGN.md section 4,
// profiles/critic_backward_kernel_stats.txt).  A workgroup spends ~12 us per plane and output channel whatever the launch,
// so the kernel needs the chip filled: 64 -> 1 at 180 workgroups and more x1.0-1.58 (x1.37 at the finest video level, B = 2),
// at 144 and fewer x0.27-0.89.  With Cout = 3 it makes three passes over every plane and loses everywhere (x0.15-0.44): those
// layers stay on the second generation.
inline bool conv_use_narrowt(const CKnobs& k, const CShape& c, bool ok, long nwg) {
  if (!ok || k.narrowt == 1) return false;
  if (k.narrowt == 2) return true;
  return c.Cout == 1 && c.T >= 7 && nwg >= 180;
}

// --------------------------------------------------------------------------------------------------------------- plan memo
// (memo_lookup: hpvg_host.h)  Every plan of one launch shape, filled at its first launch or query: a search costs 10-100 us of
// host time and shapes repeat every iteration.  direct / wino: [0] one workgroup per tile, [1] stream-K.  A narrow shape has
// its first-generation tiles in both direct slots and the second generation's geometry in n2; a wide one the rest, the
// Winograd entries only where the layer has the kernels (L == 0: no tile fits, w2.ok / n2_ok false: cannot run).
// hpvg_conv_wino_config's staging forms move plan_wino_search, and bump CKnobs::gen with them.
struct CPlans {
  Plan direct[2], wino[2];
  W2Geom w2;
  Narrow2Geom n2;
  long n2_tiles;
  bool n2_ok;
  NarrowTGeom nt;     // conv_narrowt_kernel (3x3x3 only)
  long nt_wgs;
  bool nt_ok;
};
const CPlans& conv_plans(const CKnobs& k, const CShape& c) {
  return memo_lookup<CPlans>(k.gen, c.B, c.Cin, c.Cout, c.T, c.H, c.W, c.KT, [&] {
    CPlans pl{};
    if (conv_is_narrow(c.Cin, c.Cout)) {
      pl.direct[0] = pl.direct[1] = plan_narrow_search(c);
      pl.n2_ok = plan_narrow2(c.B, c.Cin, c.Cout, c.T, c.H, c.W, c.KT, &pl.n2, &pl.n2_tiles);
      pl.nt_ok = plan_narrowt(c.B, c.Cin, c.Cout, c.T, c.H, c.W, c.KT, &pl.nt, &pl.nt_wgs);
      return pl;
    }
    for (int sk = 0; sk < 2; ++sk) {
      pl.direct[sk] = plan_conv_search(k, c, sk != 0);
      if (conv_is_wino(k, c.Cin, c.Cout)) pl.wino[sk] = plan_wino_search(k, c, sk != 0);
    }
    pl.w2 = wino2d_geom(k, c);
    return pl;
  });
}

// ------------------------------------------------------------------------------------------------ scratch, per kernel family
inline int conv_ntiles(const CShape& c, const Plan& p) { return c.B * c.T * p.nrange * p.ntw * p.gridy; }
// stream-K grid for a plan: all co-resident slots, or one workgroup per item when there are fewer items than slots
inline int conv_sk_grid(const CShape& c, const Plan& p) {
  const long items = (long)conv_ntiles(c, p) * hpvg_cdiv(c.Cin, conv_cc(c.Cin));
  const long slots = conv_slots(p.MB, p.NB);
  return (int)(items < slots ? items : slots);
}
// the stream-K schedule's partial slabs of the direct and the one-axis Winograd kernel (the other two kernels need none)
inline size_t conv_sk_ws_bytes(const CShape& c, const Plan& p) {
  return p.L ? (size_t)conv_sk_grid(c, p) * 2 * p.MB * p.NB * 16 * 256 * sizeof(float) : 0;
}

// ------------------------------------------------------------------------------------------------------------ the decision
// Where the one-axis Winograd kernel is taken.  Default threshold, measured per pyramid stage at B = 2 (tools/perf_wino.py,
// profiles/r02_perf_wino.txt): the 3x3x3 convs gain at every stage (x1.14-1.18 at stages 0-1, parity at 2, x1.08-1.32 from 3
// up); the 3x3 convs are launch / fix-up bound below ~25 K output positions (x0.75-1.0) and gain from there (x1.07-1.25 at
// stages 7-9).
inline bool conv_use_wino(const CKnobs& k, const CShape& c, bool prologue) {
  if (prologue || !conv_is_wino(k, c.Cin, c.Cout) || k.wino == 0) return false;
  if (k.wino == 2) return true;
  const long min_pos = k.min_pos >= 0 ? k.min_pos : (c.KT == 3 ? 0L : 24000L);
  return (long)c.B * c.T * c.H * c.W >= min_pos;
}
// Where the two-axis kernel is taken, of the launches conv_use_wino lets through: by size where it was measured to win.
// Whole tiles, one workgroup per CU, no stream-K: a launch takes ceil(tiles / 256)
// rounds of ~72 us (64 -> 64; w2_split_plan runs a last round that is at most half full as half / quarter tiles, 0.45-0.7 of a
// round - the rule below was measured without it and counts whole rounds), the one-axis kernel + fix-up ~100-120 us per 256 tiles' worth of work (more below one round).
// Round 3, conv_wino2r_kernel against the one-axis kernel (tools/perf_wino2.py, profiles/r03_perf_wino2r_sizes.txt; rounds =
// tiles / 256): 0.35 x0.94, 0.59 x1.12, 0.70 x1.48, 0.94 x1.43, 1.17 x0.94, 1.88 x1.36, 1.97 x1.07 (odd W), 3.23 x1.18-1.21,
// 3.94 x1.13 (odd W), 4.98 x1.37, 6.45 x1.31, 14.6 x1.33.  (Before the plane-end patch ran on twelve lanes at once the TAIL
// instance - H * W % 4 != 0 - lost below two rounds; round 2's conv_wino2d_kernel wanted three rounds filled to 88 %.)
// Rule: a single round from half a chip of tiles (the one-axis kernel pays its fix-up launch and stream-K seams there), else
// the rounds at least 60 % full on average.
inline bool conv_use_wino2d(const CKnobs& k, const W2Geom& q) {
  if (!q.ok || k.w2d == 1) return false;
  if (k.w2d == 2) return true;
  const long rounds = (q.ntl + HPVG_NUM_CU - 1) / HPVG_NUM_CU;
  if (rounds == 1) return q.ntl * 2 >= HPVG_NUM_CU;
  return (long)q.ntl * 10 >= 6L * rounds * HPVG_NUM_CU;
}

// Which kernel family runs a launch, on which plan, grid and scratch.  The launcher, its "workspace too small" step and the
// host queries all read this one answer.  The chain: narrow (second generation, then first), two-axis Winograd, one-axis
// Winograd (back to direct where no tile fits), direct; stream-K where a large enough workspace is given.
struct CDecision {
  int kind;           // hpvg_conv_fwd_kernel_kind's numbering: 0 conv_mfma_kernel, 1 conv_wino_kernel, 2 the two-axis
                      // kernels (plans->w2), 3 the narrow kernels
  int narrow_gen;     // kind 3: 3 = conv_narrowt_kernel (plans->nt), 2 = conv_narrow2_kernel (plans->n2), 1 = conv_narrow_kernel
                      // (on plan's tiles)
  const CPlans* plans;
  const Plan* plan;   // kinds 0, 1, 3; L == 0: no tile fits the shape
  bool streamk;
  int ntl, S;         // tiles, workgroups
  size_t ws_bytes;    // the scratch that launch needs
};
CDecision conv_decide(const CShape& c, bool prologue, bool fp32_out_mask, const void* ws, size_t ws_bytes) {
  const CKnobs& k = cknobs();
  CDecision d{};
  const CPlans& pl = conv_plans(k, c);
  d.plans = &pl;
  if (conv_is_narrow(c.Cin, c.Cout)) {
    d.kind = 3;
    d.plan = &pl.direct[0];
    d.narrow_gen = !k.narrow2_off && !prologue && !fp32_out_mask && pl.n2_ok ? 2 : 1;
    if (!prologue && !fp32_out_mask && conv_use_narrowt(k, c, pl.nt_ok, pl.nt_wgs)) d.narrow_gen = 3;
    d.ntl = d.S = conv_ntiles(c, *d.plan);
    return d;
  }
  bool wino = conv_use_wino(k, c, prologue);
  if (wino && conv_use_wino2d(k, pl.w2) && !fp32_out_mask) {   // (fp32 out-masks: one-axis kernel)
    d.kind = 2;
    d.ntl = pl.w2.ntl;
    d.S = d.ntl < HPVG_NUM_CU ? d.ntl : HPVG_NUM_CU;
    return d;
  }
  d.streamk = !k.sk_off && ws != nullptr;
  if (wino && pl.wino[d.streamk].L == 0) wino = false;   // no Winograd tile fits this shape: the direct kernel takes it
  const Plan* both = wino ? pl.wino : pl.direct;
  if (d.streamk && ws_bytes < conv_sk_ws_bytes(c, both[1])) d.streamk = false;   // workspace too small: the plan without stream-K
  d.kind = wino ? 1 : 0;
  d.plan = &both[d.streamk];
  d.ntl = conv_ntiles(c, *d.plan);
  d.S = d.streamk ? conv_sk_grid(c, *d.plan) : d.ntl;   // S = ntl: one data-parallel round, no stream-K part
  d.ws_bytes = d.streamk ? conv_sk_ws_bytes(c, *d.plan) : 0;
  return d;
}
// what the host queries ask: no prologue, no fp32 mask, scratch available
inline CDecision conv_decide_query(const CShape& c) { return conv_decide(c, false, false, &c, ~(size_t)0); }

// ---------------------------------------------------------------------------------------------------------------- launches
// (launch_lds: hpvg_host.h)  The operands of one hpvg_conv_fwd_* call
struct CCall {
  const float* x; const float* wp; const float* bias;
  const float* in_scale; const float* in_shift; int in_lrelu;
  float* y; int out_lrelu;
  const float* out_mask; const unsigned* mask_bits; unsigned* bits_out;
  void* ws; size_t ws_bytes;
  CShape c;
  hipStream_t s;
};

// kernel arguments of the direct, one-axis Winograd and narrow kernels
ConvFwdArgs conv_args(const CCall& q, const CDecision& d, int stagger) {
  const CShape& c = q.c;
  const Plan& p = *d.plan;
  ConvFwdArgs a{};
  a.x = q.x; a.bias = q.bias; a.in_scale = q.in_scale; a.in_shift = q.in_shift; a.mask = q.out_mask; a.y = q.y;
  a.wp = d.kind == 1 ? q.wp + direct_pack_floats(c.Cin, c.Cout, c.KT) : q.wp;   // the U fragments follow the direct pack
  a.mask_bits = q.mask_bits; a.bits_out = q.bits_out;
  a.B = c.B; a.Cin = c.Cin; a.Cout = c.Cout; a.T = c.T; a.H = c.H; a.W = c.W;
  a.Th = p.Th; a.Tw = p.Tw; a.RS = p.RS; a.PL = p.PL; a.L = p.L; a.qstride = p.qstride; a.nrange = p.nrange; a.ntw = p.ntw; a.nblocks = p.nblocks;
  a.nchunk = hpvg_cdiv(c.Cin, conv_cc(c.Cin));
  a.mbtot = hpvg_cdiv(c.Cout, 32);
  a.nj = p.nj;
  a.in_lrelu = q.in_lrelu; a.out_lrelu = q.out_lrelu;
  a.gridy = p.gridy;
  a.ntl = d.ntl;
  a.ndp = d.ntl / d.S;
  a.skbase = a.ndp * d.S;
  a.skpart = d.kind == 3 ? nullptr : (float*)q.ws;
  a.stagger = d.kind == 1 && d.S > HPVG_NUM_CU ? stagger : 0;   // only when two workgroups share a CU
  return a;
}
// ... of the two-axis Winograd kernels
Wino2Args wino2_args(const CCall& q, const W2Geom& g) {
  const CShape& c = q.c;
  Wino2Args a{};
  a.x = q.x; a.bias = q.bias; a.mask_bits = q.mask_bits; a.bits_out = q.bits_out; a.y = q.y;
  a.wp = q.wp + direct_pack_floats(c.Cin, c.Cout, c.KT) + wino_pack_floats(c.Cin, c.Cout, c.KT);
  a.B = c.B; a.Cin = c.Cin; a.Cout = c.Cout; a.T = c.T; a.H = c.H; a.W = c.W;
  a.Cq = g.Cq; a.R = g.R; a.ntq = g.ntq; a.tqw = g.tqw; a.mbtot = wino2_mb(c.Cout); a.gridy = g.gridy;
  a.nsc = g.nsc; a.ntl = g.ntl; a.PL = W2_PL; a.out_lrelu = q.out_lrelu;
  a.mbreal = hpvg_cdiv(c.Cout, 32);   // (the mask words are laid out over the layer's real m-tile count)
  return a;
}

// conv_mfma_kernel on S workgroups, then the fix-up of the tiles cut across them.  The dynamic LDS request is padded to
// 56 KB so that a third workgroup never fits on a CU: the persistent grid is sized for exactly two (four per CU: padded to
// 33 KB so that a fifth never fits).
constexpr size_t CONV_MIN_LDS = 56 * 1024;
template <int CC, int KT, int MB, int NB, int VAR>
int launch_conv_var(const ConvFwdArgs& a, const Plan& p, int S, hipStream_t s) {
  const size_t min_lds = HPVG_CONV_WGS(MB, NB) == 4 ? (size_t)33 * 1024 : CONV_MIN_LDS;
  const int rc = launch_lds<conv_mfma_kernel<CC, KT, MB, NB, VAR>>(dim3(S), dim3(256), p.lds < min_lds ? min_lds : p.lds, s, a);
  const int nsk = a.ntl - a.skbase;
  if (rc != HPVG_OK || nsk <= 0) return rc;
  hipLaunchKernelGGL(conv_fixup_kernel, dim3(nsk, MB * NB), dim3(256), 0, s, a, S, MB, NB);
  return hpvg_launch_status();
}
template <int CC, int KT, int MB, int NB>
int launch_conv_tile(const ConvFwdArgs& a, const Plan& p, int S, hipStream_t s) {
  if (a.in_scale) return launch_conv_var<CC, KT, MB, NB, VAR_PRO>(a, p, S, s);
  if (a.mask || a.mask_bits) return launch_conv_var<CC, KT, MB, NB, VAR_MASK>(a, p, S, s);
  if (a.bits_out) return launch_conv_var<CC, KT, MB, NB, VAR_BITS>(a, p, S, s);
  return launch_conv_var<CC, KT, MB, NB, VAR_PLAIN>(a, p, S, s);
}
template <int CC, int KT>
int launch_conv(const ConvFwdArgs& a, const Plan& p, int S, hipStream_t s) {
  if (p.MB == 2) {
    if (p.NB == 1) return launch_conv_tile<CC, KT, 2, 1>(a, p, S, s);
    return p.NB == 2 ? launch_conv_tile<CC, KT, 2, 2>(a, p, S, s) : launch_conv_tile<CC, KT, 2, 4>(a, p, S, s);
  }
  if (p.NB == 1) return launch_conv_tile<CC, KT, 1, 1>(a, p, S, s);
  return p.NB == 2 ? launch_conv_tile<CC, KT, 1, 2>(a, p, S, s) : launch_conv_tile<CC, KT, 1, 4>(a, p, S, s);
}

// conv_wino_kernel and its fix-up
template <int KT, int VAR, int STG>
int launch_wino_var(const ConvFwdArgs& a, const Plan& p, int S, hipStream_t s) {
  const int rc = launch_lds<conv_wino_kernel<KT, WINO_NBP, VAR, STG>>(dim3(S), dim3(256), p.lds < CONV_MIN_LDS ? CONV_MIN_LDS : p.lds, s, a);
  const int nsk = a.ntl - a.skbase;
  if (rc != HPVG_OK || nsk <= 0) return rc;
  hipLaunchKernelGGL(conv_wino_fixup_kernel, dim3(nsk, WINO_NBP * 2), dim3(256), 0, s, a, S, WINO_NBP);
  return hpvg_launch_status();
}
template <int KT, int STG>
int launch_wino_stg(const ConvFwdArgs& a, const Plan& p, int S, hipStream_t s) {
  if (a.mask || a.mask_bits) return launch_wino_var<KT, VAR_MASK, STG>(a, p, S, s);
  if (a.bits_out) return launch_wino_var<KT, VAR_BITS, STG>(a, p, S, s);
  return launch_wino_var<KT, VAR_PLAIN, STG>(a, p, S, s);
}
template <int KT>
int launch_wino(const ConvFwdArgs& a, const Plan& p, int S, hipStream_t s) {
  return p.stg == 2 ? launch_wino_stg<KT, 2>(a, p, S, s) : launch_wino_stg<KT, 1>(a, p, S, s);
}

// the two-axis kernels: conv_wino2r_kernel (only it has an odd-W instance), or the first generation with HPVG_WINO2R=0
// (sub: conv_wino2r_kernel's SUB - 0 whole tiles, 1 half tiles, 2 quarter tiles; only w2_split_plan asks for 1 or 2)
template <int VAR, bool TAIL, bool ODD>
int launch_wino2r_sub(int sub, const Wino2Args& a, int S, size_t lds, hipStream_t s) {
  if (sub == 2) return launch_lds<conv_wino2r_kernel<VAR, TAIL, ODD, 2>>(dim3(S), dim3(256), lds, s, a);
  if (sub == 1) return launch_lds<conv_wino2r_kernel<VAR, TAIL, ODD, 1>>(dim3(S), dim3(256), lds, s, a);
  return launch_lds<conv_wino2r_kernel<VAR, TAIL, ODD, 0>>(dim3(S), dim3(256), lds, s, a);
}
template <int VAR, bool TAIL>
int launch_wino2d_inst(bool w2r, int sub, const Wino2Args& a, int S, hipStream_t s) {
  const size_t lds = (size_t)3 * 12 * W2_PL * sizeof(float);   // three input buffers
  if (a.W & 1) return launch_wino2r_sub<VAR, TAIL, true>(sub, a, S, lds, s);
  if (w2r) return launch_wino2r_sub<VAR, TAIL, false>(sub, a, S, lds, s);
  return launch_lds<conv_wino2d_kernel<VAR, TAIL>>(dim3(S), dim3(256), lds, s, a);
}
template <int VAR>
int launch_wino2d_var(bool w2r, int sub, const Wino2Args& a, int S, hipStream_t s) {
  return (((long)a.H * a.W) & 3) ? launch_wino2d_inst<VAR, true>(w2r, sub, a, S, s) : launch_wino2d_inst<VAR, false>(w2r, sub, a, S, s);
}
int launch_wino2d_form(bool w2r, int sub, const Wino2Args& a, int S, hipStream_t s) {
  if (a.mask_bits) return launch_wino2d_var<VAR_MASK>(w2r, sub, a, S, s);
  if (a.bits_out) return launch_wino2d_var<VAR_BITS>(w2r, sub, a, S, s);
  return launch_wino2d_var<VAR_PLAIN>(w2r, sub, a, S, s);
}
// the whole-tile launch over the full rounds, then (w2_split_plan) the leftover tiles' parts on the same stream
int launch_wino2d(bool w2r, Wino2Args a, const W2Geom& g, int S, hipStream_t s) {
  if (g.sp_parts == 1) return launch_wino2d_form(w2r, 0, a, S, s);
  a.ntl = g.sp_full;
  const int rc = launch_wino2d_form(w2r, 0, a, HPVG_NUM_CU, s);
  if (rc != HPVG_OK) return rc;
  a.sub0 = g.sp_full;
  a.ntl = g.sp_wgs;
  return launch_wino2d_form(w2r, g.sp_parts == 4 ? 2 : 1, a, g.sp_wgs, s);
}

// the narrow kernels: one or two 32-column tiles of the 9 * Cout rows of P
template <int KT>
int launch_narrow(const ConvFwdArgs& a, const CDecision& d, hipStream_t s) {
  const int ksteps = hpvg_cdiv(a.Cin * KT, 2);
  const bool one = 9 * a.Cout <= 32;
  if constexpr (KT == 3) {
    if (d.narrow_gen == 3) {
      const NarrowTGeom& g = d.plans->nt;
      const dim3 grid((unsigned)d.plans->nt_wgs);
      const size_t lds = narrowt_lds(g);
      switch (a.Cout) {
        case 1: return launch_lds<conv_narrowt_kernel<1>>(grid, dim3(256), lds, s, a, g);
        case 2: return launch_lds<conv_narrowt_kernel<2>>(grid, dim3(256), lds, s, a, g);
        case 3: return launch_lds<conv_narrowt_kernel<3>>(grid, dim3(256), lds, s, a, g);
        default: return launch_lds<conv_narrowt_kernel<4>>(grid, dim3(256), lds, s, a, g);
      }
    }
  }
  if (d.narrow_gen == 2) {
    const Narrow2Geom& g = d.plans->n2;
    const dim3 grid((unsigned)d.plans->n2_tiles);
    const size_t lds = (size_t)(9 * a.Cout) * g.pitch * sizeof(float);
    return one ? launch_lds<conv_narrow2_kernel<KT, 1, 4>>(grid, dim3(256), lds, s, a, g, ksteps)
               : launch_lds<conv_narrow2_kernel<KT, 2, 2>>(grid, dim3(256), lds, s, a, g, ksteps);
  }
  const int pitch = (hpvg_cdiv((d.plan->Th + 2) * d.plan->RS, 32) * 32) | 1;  // odd: the 32 columns of a block land in 32 banks
  const size_t lds = (size_t)(9 * a.Cout) * pitch * sizeof(float);
  return one ? launch_lds<conv_narrow_kernel<KT, 1>>(dim3(a.ntl), dim3(256), lds, s, a, ksteps, pitch)
             : launch_lds<conv_narrow_kernel<KT, 2>>(dim3(a.ntl), dim3(256), lds, s, a, ksteps, pitch);
}

// y[b][o][t][h][w] = bias[o] + sum_{c,tap} Wp[o][c][tap] * f(x)[b][c][t+dt-pt][h+dh-1][w+dw-1]
// f = identity, or (in_scale[c]*x + in_shift[c]) followed by LeakyReLU(0.2) when in_lrelu (zero padding
// is applied AFTER f, as in the reference where f is the previous block's BatchNorm+LeakyReLU output).
// out_mask (optional, the output's shape): y *= (out_mask > 0 ? 1 : 0.2) after bias / LeakyReLU - the leaky_relu_backward of
// the layer below, fused into this conv when it runs as that layer's consumer's backward-data pass.
// ws / ws_bytes: hpvg_conv_fwd_ws_bytes() of scratch enables the stream-K schedule; with ws = NULL (or too small)
// the same kernel runs one workgroup per tile.
int conv_fwd_launch(const CCall& q) {
  const CShape& c = q.c;
  if (!q.x || !q.wp || !q.y) return HPVG_ERR_ARG;
  if (const int rc = conv_check(c)) return rc;
  if ((q.in_scale == nullptr) != (q.in_shift == nullptr)) return HPVG_ERR_ARG;
  if (q.in_scale && q.out_mask && !conv_is_narrow(c.Cin, c.Cout)) return HPVG_ERR_UNSUPPORTED;  // no caller combines prologue and mask
  const CDecision d = conv_decide(c, q.in_scale != nullptr, q.out_mask != nullptr, q.ws, q.ws_bytes);
  if (d.kind == 2) return launch_wino2d(cknobs().w2r, wino2_args(q, d.plans->w2), d.plans->w2, d.S, q.s);
  if (d.plan->L == 0) return HPVG_ERR_UNSUPPORTED;
  const ConvFwdArgs a = conv_args(q, d, cknobs().stagger);
  if (d.kind == 3) return c.KT == 3 ? launch_narrow<3>(a, d, q.s) : launch_narrow<1>(a, d, q.s);
  if (d.kind == 1) return c.KT == 3 ? launch_wino<3>(a, *d.plan, d.S, q.s) : launch_wino<1>(a, *d.plan, d.S, q.s);
  if (conv_cc(c.Cin) == 8) return c.KT == 3 ? launch_conv<8, 3>(a, *d.plan, d.S, q.s) : launch_conv<8, 1>(a, *d.plan, d.S, q.s);
  return c.KT == 3 ? launch_conv<4, 3>(a, *d.plan, d.S, q.s) : launch_conv<4, 1>(a, *d.plan, d.S, q.s);
}

// does a launch of this geometry run the two-axis Winograd kernel (and therefore read the pack's third section)?
bool wants_wino2d(const CShape& c) { return conv_check(c) == HPVG_OK && conv_decide_query(c).kind == 2; }

// w: natural layout of the LAYER weight [Cout_layer][Cin_layer][KT][3][3].
// transpose_flip = 0: pack for the forward conv (kernel Cin=Cin_layer, Cout=Cout_layer)
// transpose_flip = 1: pack for backward-data (kernel Cin=Cout_layer, Cout=Cin_layer)
int pack_weight_launch(const float* w, const float* inv_scale, float* wp, int Cin_layer, int Cout_layer, int KT, int transpose_flip,
                       bool with2d, void* stream) {
  if (!w || !wp || (KT != 1 && KT != 3) || Cin_layer < 1 || Cout_layer < 1) return HPVG_ERR_ARG;
  const int Cin_k = transpose_flip ? Cout_layer : Cin_layer;
  const int Cout_k = transpose_flip ? Cin_layer : Cout_layer;
  const long total = (long)wpack_floats(Cin_k, Cout_k, KT, with2d);
  if (conv_is_narrow(Cin_k, Cout_k)) {
    hipLaunchKernelGGL(conv_pack_narrow_kernel, dim3(hpvg_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, inv_scale, wp,
                       Cin_k, Cout_k, KT, hpvg_cdiv(9 * Cout_k, 32), hpvg_cdiv(Cin_k * KT, 2), transpose_flip, total);
    return hpvg_launch_status();
  }
  const int CC = conv_cc(Cin_k);
  hipLaunchKernelGGL(conv_pack_kernel, dim3(hpvg_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, inv_scale, wp, Cin_k, Cout_k,
                     KT * 9, CC, hpvg_cdiv(Cin_k, CC), hpvg_cdiv(Cout_k, 32), transpose_flip, (long)direct_pack_floats(Cin_k, Cout_k, KT),
                     total);
  return hpvg_launch_status();
}

// n <= HPVG_PACK_BATCH_MAX weights of one SQUARE layer shape (C -> C, C > 4) packed in one launch; flip[i] selects the
// backward-data pack for item i.  Host arrays of device pointers (copied into the kernel arguments).
int pack_batch_launch(int n, const float* const* w, float* const* wp, const int* flip, int C, int KT, bool with2d, void* stream) {
  if (n < 1 || n > HPVG_PACK_BATCH_MAX || !w || !wp || !flip || C <= 4 || (KT != 1 && KT != 3)) return HPVG_ERR_ARG;
  PackBatchArgs a;
  for (int i = 0; i < n; ++i) {
    if (!w[i] || !wp[i]) return HPVG_ERR_ARG;
    a.w[i] = w[i]; a.wp[i] = wp[i]; a.flip[i] = flip[i];
  }
  const int CC = conv_cc(C);
  const long total = (long)wpack_floats(C, C, KT, with2d);
  hipLaunchKernelGGL(conv_pack_batch_kernel, dim3(hpvg_cdiv(total, 256), n), dim3(256), 0, (hipStream_t)stream, a, C, KT * 9, CC,
                     hpvg_cdiv(C, CC), hpvg_cdiv(C, 32), (long)direct_pack_floats(C, C, KT), total);
  return hpvg_launch_status();
}

// out[0..9] of the two wide plan queries, which differ in out[4] and in the tile count
int write_plan(const Plan& p, int out4, int ntiles, int* out) {
  out[0] = p.L; out[1] = p.Tw; out[2] = p.nrange; out[3] = p.ntw; out[4] = out4; out[5] = p.NB; out[6] = p.MB;
  out[7] = p.gridy; out[8] = (int)p.lds; out[9] = ntiles;
  return HPVG_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------ entry points
extern "C" {

// A pack made WITHOUT a geometry serves every launch of the layer (all sections); the _for forms leave out the two-axis
// Winograd fragments (786 KB for 64 -> 64 x 27) unless a launch of the given geometry (kernel view: the conv's input
// B, T, H, W) reads them, and are valid for launches of that geometry only.
size_t hpvg_conv_wpack_floats(int Cin, int Cout, int KT) { return wpack_floats(Cin, Cout, KT, true); }
size_t hpvg_conv_wpack_floats_for(int Cin, int Cout, int KT, int B, int T, int H, int W) {
  return wpack_floats(Cin, Cout, KT, wants_wino2d({B, Cin, Cout, T, H, W, KT}));
}
int hpvg_conv_wants_wino2d(int B, int Cin, int Cout, int T, int H, int W, int KT) { return wants_wino2d({B, Cin, Cout, T, H, W, KT}) ? 1 : 0; }

int hpvg_conv_pack_weight_f32(const float* w, const float* inv_scale, float* wp, int Cin_layer, int Cout_layer, int KT,
                              int transpose_flip, void* stream) {
  return pack_weight_launch(w, inv_scale, wp, Cin_layer, Cout_layer, KT, transpose_flip, true, stream);
}
int hpvg_conv_pack_weight_for_f32(const float* w, const float* inv_scale, float* wp, int Cin_layer, int Cout_layer, int KT,
                                  int transpose_flip, int B, int T, int H, int W, void* stream) {
  const int Cin_k = transpose_flip ? Cout_layer : Cin_layer, Cout_k = transpose_flip ? Cin_layer : Cout_layer;
  return pack_weight_launch(w, inv_scale, wp, Cin_layer, Cout_layer, KT, transpose_flip, wants_wino2d({B, Cin_k, Cout_k, T, H, W, KT}), stream);
}
int hpvg_conv_pack_weight_batch_f32(int n, const float* const* w, float* const* wp, const int* flip, int C, int KT, void* stream) {
  return pack_batch_launch(n, w, wp, flip, C, KT, true, stream);
}
int hpvg_conv_pack_weight_batch_for_f32(int n, const float* const* w, float* const* wp, const int* flip, int C, int KT, int B, int T,
                                        int H, int W, void* stream) {
  return pack_batch_launch(n, w, wp, flip, C, KT, wants_wino2d({B, C, C, T, H, W, KT}), stream);
}

int hpvg_conv_fwd_f32(const float* x, const float* wp, const float* bias, const float* in_scale, const float* in_shift,
                      int in_lrelu, float* y, int out_lrelu, const float* out_mask, void* ws, size_t ws_bytes, int B, int Cin,
                      int Cout, int T, int H, int W, int KT, void* stream) {
  return conv_fwd_launch({x, wp, bias, in_scale, in_shift, in_lrelu, y, out_lrelu, out_mask, nullptr, nullptr, ws, ws_bytes,
                          {B, Cin, Cout, T, H, W, KT}, (hipStream_t)stream});
}

// number of 32-bit words of the 1-bit LeakyReLU mask of a [B][C][T][H][W] activation: [B][ceil(C/32)][T*H*W] (position fastest:
// the lanes of a wave hold neighbouring positions, so the word stores / loads of every conv kernel's epilogue are contiguous)
size_t hpvg_conv_mask_words(int B, int C, int T, int H, int W) { return (size_t)B * T * H * W * hpvg_cdiv(C, 32); }

// y = conv(x) (+bias) with the LeakyReLU sign mask in 1-bit form: `bits_out` (with out_lrelu; written for the consumer's
// backward-data conv) and / or `mask_bits` (read instead of a float out_mask).  Cout > 4 only (the MFMA kernel).
int hpvg_conv_fwd_bits_f32(const float* x, const float* wp, const float* bias, float* y, int out_lrelu, const unsigned* mask_bits,
                           unsigned* bits_out, void* ws, size_t ws_bytes, int B, int Cin, int Cout, int T, int H, int W, int KT,
                           void* stream) {
  if (conv_is_narrow(Cin, Cout)) return HPVG_ERR_UNSUPPORTED;
  if (mask_bits && bits_out) return HPVG_ERR_UNSUPPORTED;
  return conv_fwd_launch({x, wp, bias, nullptr, nullptr, 0, y, out_lrelu, nullptr, mask_bits, bits_out, ws, ws_bytes,
                          {B, Cin, Cout, T, H, W, KT}, (hipStream_t)stream});
}

// host only: which kernel family hpvg_conv_fwd_f32 / hpvg_conv_fwd_bits_f32 run this shape on (no prologue, no fp32 out-mask):
// 0 = direct implicit GEMM (conv_mfma_kernel), 1 = Winograd F(2,3) along W (conv_wino_kernel: 2/3 of the direct matrix-core
// work), 2 = Winograd F(2x2,3x3) (conv_wino2d_kernel: 4/9), 3 = the narrow-output kernel (Cout <= 4)
int hpvg_conv_fwd_kernel_kind(int B, int Cin, int Cout, int T, int H, int W, int KT) {
  const CShape c{B, Cin, Cout, T, H, W, KT};
  return conv_check(c) == HPVG_OK ? conv_decide_query(c).kind : HPVG_ERR_ARG;
}

// scratch the stream-K schedule of hpvg_conv_fwd_f32 wants for this shape: the larger of the direct and the one-axis kernel's
// needs, since a launch with a BatchNorm prologue or an fp32 out-mask lands there whatever conv_decide_query answers
size_t hpvg_conv_fwd_ws_bytes(int B, int Cin, int Cout, int T, int H, int W, int KT) {
  const CShape c{B, Cin, Cout, T, H, W, KT};
  if (conv_check(c) != HPVG_OK || conv_is_narrow(Cin, Cout)) return 0;
  const CKnobs& k = cknobs();
  const CPlans& pl = conv_plans(k, c);
  const size_t direct = conv_sk_ws_bytes(c, pl.direct[1]), wino = conv_use_wino(k, c, false) ? conv_sk_ws_bytes(c, pl.wino[1]) : 0;
  return direct > wino ? direct : wino;
}

// Debug/introspection: the tile plan of the direct kernel's stream-K launch (for tests and DESIGN.md tables), whichever
// kernel runs the shape; a narrow shape: conv_narrow_kernel's tiles.
// out[0..9] = L (positions per tile), Tw (band width), nrange (tiles per band plane), ntw (bands), nblocks, NB, MB, gridy,
// lds_bytes, ntiles (of one output-channel group)
int hpvg_conv_fwd_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out) {
  const CShape c{B, Cin, Cout, T, H, W, KT};
  if (!out || conv_check(c) != HPVG_OK) return HPVG_ERR_ARG;
  const Plan& p = conv_plans(cknobs(), c).direct[1];
  return write_plan(p, p.nblocks, B * T * p.nrange * p.ntw, out);
}

// host only: how a launch of this shape that runs the two-axis kernel (hpvg_conv_fwd_kernel_kind 2; any other shape:
// HPVG_ERR_UNSUPPORTED) is cut (w2_split_plan): out[0..3] = tiles of the whole-tile launch, leftover tiles, parts per leftover
// tile (1 = none, 2 = half tiles, 4 = quarter tiles), workgroups of the launch that runs the parts
int hpvg_conv_w2_split(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out) {
  const CShape c{B, Cin, Cout, T, H, W, KT};
  if (!out || conv_check(c) != HPVG_OK) return HPVG_ERR_ARG;
  const CDecision d = conv_decide_query(c);
  if (d.kind != 2) return HPVG_ERR_UNSUPPORTED;
  const W2Geom& g = d.plans->w2;
  out[0] = g.sp_full; out[1] = g.ntl - g.sp_full; out[2] = g.sp_parts; out[3] = g.sp_wgs;
  return HPVG_OK;
}

// Run-time switch of the Winograd path (tests and A/B tools; see CKnobs): mode 0 = direct kernel only, 1 = from
// `min_positions` output positions up, 2 = every eligible launch; 3 / 4: every eligible launch AND one staging form forced
// (rows as in memory / halo'd bands); 5: every eligible launch, the two-axis kernel wherever it can run; 3 / 4 / 6: the
// one-axis kernel only.  A negative argument leaves that setting alone.  Returns the mode in force, or HPVG_ERR_UNSUPPORTED
// when the library was started with HPVG_WINO=0 (packs carry no U fragments).
int hpvg_conv_wino_config(int mode, long min_positions) {
  CKnobs& k = cknobs();
  if (k.env_wino == 0) return HPVG_ERR_UNSUPPORTED;
  if (mode >= 0) {
    const int stg = mode == 3 ? 2 : (mode == 4 ? 1 : 0);
    if (stg != k.stg) ++k.gen;
    k.wino = mode > 2 ? 2 : mode;
    k.stg = stg;
    k.w2d = mode == 5 ? 2 : (mode == 3 || mode == 4 || mode == 6 ? 1 : 0);
  }
  if (min_positions >= 0) k.min_pos = min_positions;
  if (k.wino == 2 && k.w2d == 2) return 5;
  if (k.wino == 2 && k.stg) return k.stg == 2 ? 3 : 4;
  if (k.wino == 2 && k.w2d == 1) return 6;
  return k.wino;
}

// Debug/introspection: the tile plan conv_wino_kernel would run this shape with (whether or not the launch picks it):
// out[0..9] = L, Tw, nrange, ntw, RS, NBP, m-tiles per workgroup, gridy, lds_bytes, ntiles; HPVG_ERR_UNSUPPORTED when the
// layer is not eligible (Cin < 8, Cout <= 32) or no tile fits.
int hpvg_conv_wino_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out) {
  const CShape c{B, Cin, Cout, T, H, W, KT};
  if (!out || conv_check(c) != HPVG_OK) return HPVG_ERR_ARG;
  const Plan& p = conv_plans(cknobs(), c).wino[1];   // (not eligible: never searched)
  return p.L ? write_plan(p, p.RS, conv_ntiles(c, p), out) : HPVG_ERR_UNSUPPORTED;
}

// Debug/introspection: the tile plan of the narrow-output kernel (conv_narrow2_kernel) for tests: out[0..6] = RS, Th, nth,
// nb, npos, G, pitch, then nb triples (window start, first output column, output columns).  Returns HPVG_ERR_UNSUPPORTED
// when the shape runs on the first-generation kernel instead (HPVG_NARROW2 aside).
int hpvg_conv_narrow_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out) {
  const CShape c{B, Cin, Cout, T, H, W, KT};
  if (!out || conv_check(c) != HPVG_OK) return HPVG_ERR_ARG;
  const CPlans& pl = conv_plans(cknobs(), c);   // (not narrow: n2_ok stays false)
  if (!pl.n2_ok) return HPVG_ERR_UNSUPPORTED;
  const Narrow2Geom& g = pl.n2;
  out[0] = g.RS; out[1] = g.Th; out[2] = g.nth; out[3] = g.nb; out[4] = g.npos; out[5] = g.G; out[6] = g.pitch;
  for (int k = 0; k < g.nb; ++k) { out[7 + 3 * k] = g.ws[k]; out[8 + 3 * k] = g.ob[k]; out[9 + 3 * k] = g.on[k]; }
  return HPVG_OK;
}

// host only: the tile plan of conv_narrowt_kernel (narrow output, time taps in N) whether or not the launch picks it:
// out[0..8] = RS, Th, nth, nb, npos, G, pitch, lds_bytes, 1 when a plain launch of this shape runs on it in the mode in
// force (else 0), then nb triples (window start, first output column, output columns).  HPVG_ERR_UNSUPPORTED when the kernel
// cannot run the shape (not 3x3x3, Cout > 4, odd Cin, W < 4, not a narrow layer).
int hpvg_conv_narrowt_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out) {
  const CShape c{B, Cin, Cout, T, H, W, KT};
  if (!out || conv_check(c) != HPVG_OK) return HPVG_ERR_ARG;
  const CPlans& pl = conv_plans(cknobs(), c);   // (not narrow: nt_ok stays false)
  if (!pl.nt_ok) return HPVG_ERR_UNSUPPORTED;
  const NarrowTGeom& g = pl.nt;
  out[0] = g.RS; out[1] = g.Th; out[2] = g.nth; out[3] = g.nb; out[4] = g.npos; out[5] = g.G; out[6] = g.pitch;
  out[7] = (int)narrowt_lds(g);
  out[8] = conv_decide_query(c).narrow_gen == 3 ? 1 : 0;
  for (int k = 0; k < g.nb; ++k) { out[9 + 3 * k] = g.ws[k]; out[10 + 3 * k] = g.ob[k]; out[11 + 3 * k] = g.on[k]; }
  return HPVG_OK;
}

// Run-time form of HPVG_NARROWT (tests and A/B tools): 0 = conv_narrowt_kernel by size, 1 = never, 2 = wherever it can run;
// a negative argument leaves the setting alone.  Returns the mode in force.
int hpvg_conv_narrowt_config(int mode) {
  CKnobs& k = cknobs();
  if (mode > 2) return HPVG_ERR_ARG;
  if (mode >= 0) k.narrowt = mode;
  return k.narrowt;
}

#ifdef HPVG_TRACE
int hpvg_debug_phase_read(unsigned long long* host_out, int n) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_phase), sizeof(unsigned long long) * 4 * n) == hipSuccess ? 0 : -4;
}
int hpvg_debug_trace_read(unsigned long long* host_out, int n) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_trace), sizeof(unsigned long long) * 4 * n) == hipSuccess ? 0 : -4;
}
#endif

}  // extern "C"
