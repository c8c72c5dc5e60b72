// hp-vae-gan_amd - tap-generic 'same' convolutions for gfx950: K x K (2-D) and K x K x K (3-D) taps, K in {3, 5, 7}, stride 1,
// zero padding K / 2 (the reference's --ker-size; modules/networks_3d.py:51,63,175 with ker_size != 3).  Everything runs on
// the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32): results are fp32 fma chains in a fixed order.
//
// Forward / backward-data (convk_fwd_kernel), an implicit GEMM in the view of conv_mfma.hip:
//   M = output channels (32 per MFMA tile, 1 or 2 tiles per workgroup), N = the positions of a TH x 32 spatial tile of one
//   output plane, flattened with the LDS row stride RS = 32 + 2h so that a tap (dh, dw) is the constant offset dh * RS + dw
//   (the 2h columns between rows are computed and dropped), K = (tap, input channel).
//   Per 16-channel chunk and time tap the input plane tile with its zero halo is staged through LDS; every wave owns 4 of
//   the 16 position tiles and all M tiles (4 or 8 accumulators), so one A fragment serves four MFMAs.  The A fragments come
//   from a per-launch pack of the weight in the workspace ([m tile][tap][channel pair][lane]: one coalesced 256-byte load
//   per fragment, zero rows / channels past the layer's), written by convk_pack_kernel on the same stream; the flipped,
//   transposed weight of the backward-data conv is just another pack.
// Weight gradient (convk_wgrad_kernel): M = 32 output channels, N = 32 input channels, K = positions.  A workgroup owns one
//   (dt, dh) pair of taps, a 64 x 64 channel block (one 32 x 32 tile per wave) and every S-th position tile; each wave keeps
//   the K accumulators of dw = 0 .. K-1 in registers over all its tiles (the dy fragment of a position pair serves K MFMAs
//   on x fragments shifted by one column each).  The S partial sums go through the workspace and convk_reduce_kernel adds
//   them in the order s = 0 .. S-1: no float atomics, the same bits on every launch.
// All global accesses are dword wide and bounds-checked, so 4-byte alignment of the tensors is enough and nothing outside a
// tensor is touched.
#include "hpvg_common.h"
#include "hpvg_host.h"
#include "hpvg.h"

namespace {

constexpr int KF_TW = 32;     // output columns per tile
constexpr int KF_NT = 16;     // 32-position MFMA tiles per workgroup (4 per wave)
constexpr int KF_CC = 16;     // input channels staged per chunk
constexpr int KF_SU = 4;      // staging loads in flight per thread (more would cost the third wave per SIMD)

template <int K> struct KFwd {
  static constexpr int HALO = K / 2;
  static constexpr int RS = KF_TW + 2 * HALO;                      // LDS row stride
  static constexpr int TH = (KF_NT * 32) / RS;                     // output rows per tile (15 / 14 / 13)
  static constexpr int ROWS = TH + 2 * HALO;                       // staged rows
  // channel stride: position 511 plus the farthest tap.  Only the first ROWS * RS floats of a channel are staged; the tail
  // is never written and IS read, uninitialised, by lanes whose position lies in the dropped columns (col >= 32) or rows
  // (r >= TH).  That is safe: an MFMA output column depends on its own B column alone, and the epilogue stores no such
  // column; a kept position (r < TH, col < 32) reads at most (ROWS - 1) * RS + RS - 1, inside the staged part.
  static constexpr int CS = KF_NT * 32 + (K - 1) * RS + (K - 1);
  static_assert(ROWS * RS <= CS, "staged tile must fit the channel stride");
};

// wp[((mt * ntaps + tap) * KK2 + kk) * 64 + lane] = W(o = 32 mt + (lane & 31), c = 2 kk + (lane >> 5), tap), 0 outside
__global__ __launch_bounds__(256) void convk_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout,
                                                         int ntaps, int KK2, int MTtot, int flip) {
  const long n = (long)MTtot * ntaps * KK2 * 64;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int lane = (int)(i & 63);
    long r = i >> 6;
    const int kk = (int)(r % KK2);
    r /= KK2;
    const int tap = (int)(r % ntaps);
    const int mt = (int)(r / ntaps);
    const int o = mt * 32 + (lane & 31), c = 2 * kk + (lane >> 5);
    float v = 0.f;
    if (o < Cout && c < Cin)
      v = flip ? w[((long)c * Cout + o) * ntaps + (ntaps - 1 - tap)] : w[((long)o * Cin + c) * ntaps + tap];
    wp[i] = v;
  }
}

template <int K, int MT>
__global__ __launch_bounds__(256, 2) void convk_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                        const float* __restrict__ bias, float* __restrict__ y, int out_lrelu,
                                                        const float* __restrict__ out_mask, int Cin, int Cout, int T, int H, int W,
                                                        int KT, int nth, int ntw, int KK2) {
  typedef KFwd<K> G;
  constexpr int HALO = G::HALO, RS = G::RS, TH = G::TH, ROWS = G::ROWS, CS = G::CS, NPW = KF_NT / 4, NT2 = K * K;
  __shared__ float lds[KF_CC * CS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  int id = blockIdx.x;
  const int tw = id % ntw;
  id /= ntw;
  const int th = id % nth;
  id /= nth;
  const int t = id % T;
  const int b = id / T;
  const int h0 = th * TH, w0 = tw * KF_TW;
  const int mt0 = blockIdx.y * MT;
  const long HW = (long)H * W;
  const long mstride = (long)KT * NT2 * KK2 * 64;       // floats between the packs of two M tiles

  f32x16 acc[MT][NPW];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NPW; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[m][n][j] = 0.f;

  for (int c0 = 0; c0 < Cin; c0 += KF_CC) {
    const int cc = min(KF_CC, Cin - c0);
    const int kkn = (cc + 1) >> 1;
    for (int dt = 0; dt < KT; ++dt) {
      const int tin = t + dt - KT / 2;
      if (tin < 0 || tin >= T) continue;          // the whole plane is zero padding (uniform over the workgroup)
      __syncthreads();
      const float* xb = x + (((long)b * Cin + c0) * T + tin) * HW;
      // KF_SU loads in flight per thread: an out-of-tile element reads element 0 of the tensor (always there) and is
      // replaced by zero afterwards, so no load sits behind a branch
      const int nstage = 2 * kkn * ROWS * RS;
      for (int base = tid; base < nstage; base += 256 * KF_SU) {
        float v[KF_SU];
        bool ok[KF_SU];
#pragma unroll
        for (int u = 0; u < KF_SU; ++u) {
          const int idx = base + u * 256;
          const int c = idx / (ROWS * RS), rem = idx - c * (ROWS * RS);
          const int r = rem / RS, col = rem - r * RS;
          const int hh = h0 + r - HALO, ww = w0 + col - HALO;
          ok[u] = idx < nstage && c < cc && hh >= 0 && hh < H && ww >= 0 && ww < W;
          v[u] = ok[u] ? xb[(long)c * T * HW + (long)hh * W + ww] : x[0];
        }
#pragma unroll
        for (int u = 0; u < KF_SU; ++u) {
          const int idx = base + u * 256;
          if (idx < nstage) {
            const int c = idx / (ROWS * RS), rem = idx - c * (ROWS * RS);
            lds[c * CS + rem] = ok[u] ? v[u] : 0.f;
          }
        }
      }
      __syncthreads();
      const float* wq = wp + ((long)(mt0 * KT + dt) * NT2 * KK2 + (c0 >> 1)) * 64 + lane;
      const float* bq = lds + half * CS + wave * 32 + l31;
      const int total = NT2 * kkn;
      float a_cur[MT], a_nxt[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) a_cur[m] = wq[m * mstride];
      int tap = 0, kk = 0;
      for (int it = 0; it < total; ++it) {
        const int off = (tap / K) * RS + (tap % K) + 2 * kk * CS;
        int ntap = tap, nkk = kk + 1;
        if (nkk == kkn) {
          nkk = 0;
          ++ntap;
        }
        if (it + 1 < total) {
#pragma unroll
          for (int m = 0; m < MT; ++m) a_nxt[m] = wq[m * mstride + ((long)ntap * KK2 + nkk) * 64];
        }
        float bf[NPW];
#pragma unroll
        for (int n = 0; n < NPW; ++n) bf[n] = bq[off + n * 128];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < NPW; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[m], bf[n], acc[m][n], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < MT; ++m) a_cur[m] = a_nxt[m];
        tap = ntap;
        kk = nkk;
      }
    }
  }

  // epilogue: C/D map of the 32x32 MFMA: column = lane & 31 (position), row = (j & 3) + 8 (j >> 2) + 4 (lane >> 5) (channel)
#pragma unroll
  for (int n = 0; n < NPW; ++n) {
    const int p = (wave + 4 * n) * 32 + l31;
    const int r = p / RS, col = p - r * RS;
    const int hh = h0 + r, ww = w0 + col;
    if (r >= TH || col >= KF_TW || hh >= H || ww >= W) continue;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int o = (mt0 + m) * 32 + (j & 3) + 8 * (j >> 2) + 4 * half;
        if (o >= Cout) continue;
        const long at = (((long)b * Cout + o) * T + t) * HW + (long)hh * W + ww;
        float v = acc[m][n][j];
        if (bias) v += bias[o];
        if (out_lrelu) v = hpvg_lrelu(v);
        if (out_mask) v *= out_mask[at] > 0.f ? 1.f : HPVG_LRELU_SLOPE;
        y[at] = v;
      }
    }
  }
}

constexpr int KW_TW = 32;     // dy columns per position tile
constexpr int KW_TH = 4;      // dy rows per position tile
constexpr int KW_MAX_SPLIT = 64;
constexpr int KW_SU = 8;      // staging loads in flight per thread

template <int K> struct KWgrad {
  static constexpr int HALO = K / 2;
  static constexpr int RS = KW_TW + 2 * HALO;
  static constexpr int DS = KW_TH * KW_TW + 1;     // odd channel strides: the 32 channels of a fragment fall on 32 banks
  static constexpr int XS = KW_TH * RS + 1;
  static constexpr size_t LDS_BYTES = (size_t)64 * (DS + XS) * sizeof(float);
};

template <int K>
__global__ __launch_bounds__(256) void convk_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          float* __restrict__ part, int B, int Cin, int Cout, int T, int H, int W,
                                                          int KT, int nth, int ntw, int ncb) {
  typedef KWgrad<K> G;
  constexpr int HALO = G::HALO, RS = G::RS, DS = G::DS, XS = G::XS, TH = KW_TH, TW = KW_TW;
  extern __shared__ float lds[];
  float* dyl = lds;
  float* xl = lds + 64 * DS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int dt = blockIdx.x / K, dh = blockIdx.x % K;
  const int ob = blockIdx.y / ncb, cb = blockIdx.y % ncb;
  const int s = blockIdx.z, S = gridDim.z;
  const int ot = wave & 1, ct = wave >> 1;
  const bool active = (ob * 64 + ot * 32 < Cout) && (cb * 64 + ct * 32 < Cin);
  const long HW = (long)H * W;
  const int nitems = B * T * nth * ntw;

  f32x16 acc[K];
#pragma unroll
  for (int d = 0; d < K; ++d)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[d][j] = 0.f;

  for (int item = s; item < nitems; item += S) {
    int id = item;
    const int tw = id % ntw;
    id /= ntw;
    const int th = id % nth;
    id /= nth;
    const int t = id % T;
    const int b = id / T;
    const int tin = t + dt - KT / 2;
    if (tin < 0 || tin >= T) continue;          // x's plane is zero padding (uniform over the workgroup)
    const int h0 = th * TH, w0 = tw * TW;
    __syncthreads();
    // KW_SU loads in flight per thread (see convk_fwd_kernel)
    static_assert((64 * TH * TW) % (256 * KW_SU) == 0, "the dy staging loop is unrolled by KW_SU without a tail");
    for (int base = tid; base < 64 * TH * TW; base += 256 * KW_SU) {
      float v[KW_SU];
      bool ok[KW_SU];
#pragma unroll
      for (int u = 0; u < KW_SU; ++u) {
        const int idx = base + u * 256;
        const int o = idx / (TH * TW), rem = idx - o * (TH * TW);
        const int r = rem / TW, col = rem - r * TW;
        const int go = ob * 64 + o, hh = h0 + r, ww = w0 + col;
        ok[u] = go < Cout && hh < H && ww < W;
        v[u] = ok[u] ? dy[(((long)b * Cout + go) * T + t) * HW + (long)hh * W + ww] : dy[0];
      }
#pragma unroll
      for (int u = 0; u < KW_SU; ++u) {
        const int idx = base + u * 256;
        const int o = idx / (TH * TW), rem = idx - o * (TH * TW);
        dyl[o * DS + rem] = ok[u] ? v[u] : 0.f;
      }
    }
    for (int base = tid; base < 64 * TH * RS; base += 256 * KW_SU) {
      float v[KW_SU];
      bool ok[KW_SU];
#pragma unroll
      for (int u = 0; u < KW_SU; ++u) {
        const int idx = base + u * 256;
        const int c = idx / (TH * RS), rem = idx - c * (TH * RS);
        const int r = rem / RS, col = rem - r * RS;
        const int gc = cb * 64 + c, hh = h0 + r + dh - HALO, ww = w0 + col - HALO;
        ok[u] = idx < 64 * TH * RS && gc < Cin && hh >= 0 && hh < H && ww >= 0 && ww < W;
        v[u] = ok[u] ? x[(((long)b * Cin + gc) * T + tin) * HW + (long)hh * W + ww] : x[0];
      }
#pragma unroll
      for (int u = 0; u < KW_SU; ++u) {
        const int idx = base + u * 256;
        const int c = idx / (TH * RS), rem = idx - c * (TH * RS);
        if (idx < 64 * TH * RS) xl[c * XS + rem] = ok[u] ? v[u] : 0.f;
      }
    }
    __syncthreads();
    if (active) {
      const float* ap = dyl + (ot * 32 + l31) * DS + half;
      const float* bp = xl + (ct * 32 + l31) * XS + half;
#pragma unroll
      for (int r = 0; r < TH; ++r) {
#pragma unroll 4
        for (int cp = 0; cp < TW / 2; ++cp) {
          const float a = ap[r * TW + 2 * cp];
#pragma unroll
          for (int d = 0; d < K; ++d)
            acc[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[r * RS + 2 * cp + d], acc[d], 0, 0, 0);
        }
      }
    }
  }

  if (active) {
    const int ntaps = KT * K * K;
    const int gc = cb * 64 + ct * 32 + l31;
    if (gc < Cin) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int go = ob * 64 + ot * 32 + (j & 3) + 8 * (j >> 2) + 4 * half;
        if (go >= Cout) continue;
        float* q = part + (((long)s * Cout + go) * Cin + gc) * ntaps + (long)(dt * K + dh) * K;
#pragma unroll
        for (int d = 0; d < K; ++d) q[d] = acc[d][j];
      }
    }
  }
}

// dw[i] (+)= part[0][i] + part[1][i] + ... in that order
__global__ __launch_bounds__(256) void convk_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, long n, int S,
                                                           int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v = part[i];
  for (int s = 1; s < S; ++s) v += part[(long)s * n + i];
  dw[i] = accumulate ? dw[i] + v : v;
}

int convk_check(int B, int Cin, int Cout, int T, int H, int W, int KT, int K) {
  if (K != 3 && K != 5 && K != 7) return HPVG_ERR_ARG;
  if (KT != 1 && KT != K) return HPVG_ERR_ARG;
  if (B < 1 || Cin < 1 || Cout < 1 || T < 1 || H < 1 || W < 1) return HPVG_ERR_ARG;
  if (KT == 1 && T != 1) return HPVG_ERR_ARG;
  return HPVG_OK;
}

int convk_ws_check(const void* ws, size_t ws_bytes, size_t need) {
  if (ws == nullptr || ((uintptr_t)ws & 15) != 0 || ws_bytes < need) return HPVG_ERR_WORKSPACE;
  return HPVG_OK;
}

inline int fwd_mt(int Cout) { return Cout > 32 ? 2 : 1; }
// M tiles per workgroup of a launch (the pack holds fwd_mttot(Cout) tiles either way, and an output's sum has the same order
// with both).  By size: two (one staged input tile serves 64 output channels) once the two-tile grid has more workgroups than
// the chip has CUs; up to that one: twice the workgroups, each with half the MFMAs.  Measured on the 64 -> 64 layer at K = 5,
// B = 2 (profiles/conv_taps_perf.txt): one tile wins up to 200 two-tile workgroups (1.20 against 1.65 ms at 120), two tiles
// from 420 on (2.59 against 2.95 ms; 10.3 against 12.6 ms at 2288).
int g_fwd_mt_mode = 0;     // hpvg_convk_fwd_mt_config
inline int fwd_tiles_per_wg(long tiles, int Cout) {
  if (fwd_mt(Cout) == 1 || g_fwd_mt_mode == 1) return 1;
  if (g_fwd_mt_mode == 2) return 2;
  return tiles * hpvg_cdiv(Cout, 64) > HPVG_NUM_CU ? 2 : 1;
}
inline int fwd_mttot(int Cout) { return hpvg_cdiv(Cout, 32 * fwd_mt(Cout)) * fwd_mt(Cout); }

template <int K>
int convk_fwd_launch(const float* x, const float* wp, const float* bias, float* y, int out_lrelu, const float* out_mask, int B,
                     int Cin, int Cout, int T, int H, int W, int KT, hipStream_t s) {
  const int nth = hpvg_cdiv(H, KFwd<K>::TH), ntw = hpvg_cdiv(W, KF_TW), KK2 = (Cin + 1) / 2;
  const long tiles = (long)B * T * nth * ntw;
  if (tiles >= (1L << 24)) return HPVG_ERR_UNSUPPORTED;   // grid.x * 256 threads must stay below 2^32
  const int mt = fwd_tiles_per_wg(tiles, Cout);
  const dim3 grid((unsigned)tiles, (unsigned)hpvg_cdiv(Cout, 32 * mt));
  if (mt == 2)
    hipLaunchKernelGGL((convk_fwd_kernel<K, 2>), grid, dim3(256), 0, s, x, wp, bias, y, out_lrelu, out_mask, Cin, Cout, T, H, W, KT,
                       nth, ntw, KK2);
  else
    hipLaunchKernelGGL((convk_fwd_kernel<K, 1>), grid, dim3(256), 0, s, x, wp, bias, y, out_lrelu, out_mask, Cin, Cout, T, H, W, KT,
                       nth, ntw, KK2);
  return hpvg_launch_status();
}

// position splits of the weight gradient: enough workgroups for two per CU, never more than there are position tiles
int wgrad_split(int B, int Cin, int Cout, int T, int H, int W, int KT, int K) {
  const long items = (long)B * T * hpvg_cdiv(H, KW_TH) * hpvg_cdiv(W, KW_TW);
  const long groups = (long)KT * K * hpvg_cdiv(Cout, 64) * hpvg_cdiv(Cin, 64);
  long S = (2 * HPVG_NUM_CU + groups - 1) / groups;
  if (S > KW_MAX_SPLIT) S = KW_MAX_SPLIT;
  if (S > items) S = items;
  return S < 1 ? 1 : (int)S;
}

template <int K>
int convk_wgrad_launch(const float* dy, const float* x, float* part, int S, int B, int Cin, int Cout, int T, int H, int W, int KT,
                       hipStream_t s) {
  const int nth = hpvg_cdiv(H, KW_TH), ntw = hpvg_cdiv(W, KW_TW), ncb = hpvg_cdiv(Cin, 64);
  const dim3 grid((unsigned)(KT * K), (unsigned)(hpvg_cdiv(Cout, 64) * ncb), (unsigned)S);
  return launch_lds<convk_wgrad_kernel<K>>(grid, dim3(256), KWgrad<K>::LDS_BYTES, s, dy, x, part, B, Cin, Cout, T, H, W, KT, nth,
                                           ntw, ncb);
}

}  // namespace

extern "C" {

int hpvg_convk_fwd_mt_config(int mode) {
  if (mode >= 0 && mode <= 2) g_fwd_mt_mode = mode;
  return g_fwd_mt_mode;
}

size_t hpvg_convk_fwd_ws_bytes(int B, int Cin, int Cout, int T, int H, int W, int KT, int K) {
  if (convk_check(B, Cin, Cout, T, H, W, KT, K) != HPVG_OK) return 0;
  return (size_t)fwd_mttot(Cout) * KT * K * K * ((Cin + 1) / 2) * 64 * sizeof(float);
}

int hpvg_convk_fwd_f32(const float* x, const float* w, const float* bias, float* y, int out_lrelu, const float* out_mask, int flip,
                       void* ws, size_t ws_bytes, int B, int Cin, int Cout, int T, int H, int W, int KT, int K, void* stream) {
  int rc = convk_check(B, Cin, Cout, T, H, W, KT, K);
  if (rc != HPVG_OK) return rc;
  if (!x || !w || !y) return HPVG_ERR_ARG;
  if ((long)T * H * W >= (1L << 31)) return HPVG_ERR_UNSUPPORTED;
  rc = convk_ws_check(ws, ws_bytes, hpvg_convk_fwd_ws_bytes(B, Cin, Cout, T, H, W, KT, K));
  if (rc != HPVG_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* wp = (float*)ws;
  const int ntaps = KT * K * K, KK2 = (Cin + 1) / 2, mttot = fwd_mttot(Cout);
  const long n = (long)mttot * ntaps * KK2 * 64;
  const int pblocks = (int)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256);
  hipLaunchKernelGGL(convk_pack_kernel, dim3(pblocks), dim3(256), 0, s, w, wp, Cin, Cout, ntaps, KK2, mttot, flip ? 1 : 0);
  rc = hpvg_launch_status();
  if (rc != HPVG_OK) return rc;
  switch (K) {
    case 3: return convk_fwd_launch<3>(x, wp, bias, y, out_lrelu, out_mask, B, Cin, Cout, T, H, W, KT, s);
    case 5: return convk_fwd_launch<5>(x, wp, bias, y, out_lrelu, out_mask, B, Cin, Cout, T, H, W, KT, s);
    default: return convk_fwd_launch<7>(x, wp, bias, y, out_lrelu, out_mask, B, Cin, Cout, T, H, W, KT, s);
  }
}

size_t hpvg_convk_bwd_weight_ws_bytes(int B, int Cin, int Cout, int T, int H, int W, int KT, int K) {
  if (convk_check(B, Cin, Cout, T, H, W, KT, K) != HPVG_OK) return 0;
  const size_t n = (size_t)Cout * Cin * KT * K * K;
  return ((size_t)wgrad_split(B, Cin, Cout, T, H, W, KT, K) * n * sizeof(float) + 15) & ~(size_t)15;
}

int hpvg_convk_bwd_weight_f32(const float* dy, const float* x, float* dw, int accumulate, void* ws, size_t ws_bytes, int B, int Cin,
                              int Cout, int T, int H, int W, int KT, int K, void* stream) {
  int rc = convk_check(B, Cin, Cout, T, H, W, KT, K);
  if (rc != HPVG_OK) return rc;
  if (!dy || !x || !dw) return HPVG_ERR_ARG;
  if ((long)T * H * W >= (1L << 31) || (long)B * T * hpvg_cdiv(H, KW_TH) * hpvg_cdiv(W, KW_TW) > 0x7fffffffL) return HPVG_ERR_UNSUPPORTED;
  rc = convk_ws_check(ws, ws_bytes, hpvg_convk_bwd_weight_ws_bytes(B, Cin, Cout, T, H, W, KT, K));
  if (rc != HPVG_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  const int S = wgrad_split(B, Cin, Cout, T, H, W, KT, K);
  switch (K) {
    case 3: rc = convk_wgrad_launch<3>(dy, x, part, S, B, Cin, Cout, T, H, W, KT, s); break;
    case 5: rc = convk_wgrad_launch<5>(dy, x, part, S, B, Cin, Cout, T, H, W, KT, s); break;
    default: rc = convk_wgrad_launch<7>(dy, x, part, S, B, Cin, Cout, T, H, W, KT, s); break;
  }
  if (rc != HPVG_OK) return rc;
  const long n = (long)Cout * Cin * KT * K * K;
  hipLaunchKernelGGL(convk_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, dw, n, S, accumulate ? 1 : 0);
  return hpvg_launch_status();
}

}  // extern "C"
