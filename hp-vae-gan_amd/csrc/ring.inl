// Rings on the sampling path (generate --wrap): the circular pad in front of every generator conv and the linear resize between
// levels that interpolates across the seam.  The contracts are written out at hpvg_ring_pad_f32 and hpvg_upsample_linear_ring_f32
// in hpvg.h; this file is one way to compute them.  Included by elementwise.hip (lin_coef, ew_blocks and upsample_fwd_kernel are
// its own).
//
// Both are pure data movement as far as the machine is concerned: the pad reads NC T H W floats and writes NC (T + 2 pt) (H + 2 ph)
// (W + 2 pw); the resize reads the source once through the caches (8 taps per output, neighbouring outputs share them) and writes
// the output once.
namespace {

struct RingPadGeom {
  int T, H, W;      // source sides
  int dT, dH, dW;   // destination sides: T + 2 pt, ...
  int t0, h0, w0;   // the source index of destination index 0 per axis: mod(-p, side)
};

// the non-negative modulus
inline int ring_mod(long a, int n) {
  const long r = a % n;
  return (int)(r < 0 ? r + n : r);
}

// The value of destination element i and the 3 after it, by decoding i once and carrying w -> h -> t -> c; the source index of
// every axis is carried with it (wrapping at its side, restarting at t0 / h0 / w0 when its destination index restarts).
__device__ __forceinline__ void ring_pad_gather(const float* __restrict__ x, const RingPadGeom& g, long i, long n, int count,
                                                float* v) {
  long r = i;
  int w = (int)(r % g.dW); r /= g.dW;
  int h = (int)(r % g.dH); r /= g.dH;
  int t = (int)(r % g.dT);
  long c = r / g.dT;
  int sw = (g.w0 + w) % g.W, sh = (g.h0 + h) % g.H, st = (g.t0 + t) % g.T;
  const long svol = (long)g.T * g.H * g.W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < count && i + k < n) v[k] = x[c * svol + ((long)st * g.H + sh) * g.W + sw];
    if (++sw == g.W) sw = 0;
    if (++w == g.dW) {
      w = 0; sw = g.w0;
      if (++sh == g.H) sh = 0;
      if (++h == g.dH) {
        h = 0; sh = g.h0;
        if (++st == g.T) st = 0;
        if (++t == g.dT) { t = 0; st = g.t0; ++c; }
      }
    }
  }
}

// out[c][t][y][x] = x[c][mod(t - pt, T)][mod(y - ph, H)][mod(x - pw, W)].  Indexed by destination: item q < nvec writes the 16-byte
// aligned group of 4 elements that starts at head + 4 q with one store; item nvec writes the `head` elements in front of the first
// aligned group and item nvec + 1 the up to 3 elements behind the last one, element by element.  The shifted source is read per
// element (every read lies inside x by construction).  n < 2^31.
__global__ __launch_bounds__(256) void ring_pad_kernel(const float* __restrict__ x, float* __restrict__ out, long n, int head,
                                                        long nvec, RingPadGeom g) {
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nvec + 2; q += (long)gridDim.x * 256) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (q < nvec) {
      const long i = head + 4 * q;
      ring_pad_gather(x, g, i, n, 4, v);
      *reinterpret_cast<float4*>(out + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      const long i = q == nvec ? 0 : head + 4 * nvec;
      const int count = q == nvec ? head : (int)(n - i);
      ring_pad_gather(x, g, i, n, count, v);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < count) out[i + k] = v[k];
    }
  }
}

// A ring axis of S source and O output positions: source coordinate o S / O in exact integers, i0 its floor, f the remainder over
// O, i1 the next position round the ring.  For O = k S the remainder is (o mod k) S: the weights depend on o mod k only, and a
// roll of the source by r is a roll of the output by k r, bit for bit.
__device__ __forceinline__ Lin ring_coef(int o, int S, int O) {
  const long p = (long)o * S;
  const int i0 = (int)(p / O);
  const float f = (float)(int)(p - (long)i0 * O) / (float)O;
  return Lin{i0, i0 + 1 == S ? 0 : i0 + 1, 1.f - f, f};
}

// y[bc][to][ho][wo]: upsample_fwd_kernel with ring_coef on the flagged axes (bit 0: t, 1: h, 2: w) - the same taps, products and
// order of additions
__global__ __launch_bounds__(256) void upsample_ring_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long BC, int Ti,
                                                                 int Hi, int Wi, int To, int Ho, int Wo, float st, float sh, float sw,
                                                                 int rings) {
  const long n = BC * To * Ho * Wo;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    long r = i;
    const int wo = r % Wo; r /= Wo;
    const int ho = r % Ho; r /= Ho;
    const int to = r % To; r /= To;
    const float* xp = x + r * ((long)Ti * Hi * Wi);
    const Lin lt = (rings & 1) ? ring_coef(to, Ti, To) : lin_coef(to, Ti, st);
    const Lin lh = (rings & 2) ? ring_coef(ho, Hi, Ho) : lin_coef(ho, Hi, sh);
    const Lin lw = (rings & 4) ? ring_coef(wo, Wi, Wo) : lin_coef(wo, Wi, sw);
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int ti = a ? lt.i1 : lt.i0;
      const float wt = a ? lt.w1 : lt.w0;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int hi = b ? lh.i1 : lh.i0;
        const float wh = b ? lh.w1 : lh.w0;
        const float* row = xp + ((long)ti * Hi + hi) * Wi;
        acc += wt * wh * (lw.w0 * row[lw.i0] + lw.w1 * row[lw.i1]);
      }
    }
    y[i] = acc;
  }
}

}  // namespace

extern "C" {

int hpvg_ring_pad_f32(const float* x, long NC, int T, int H, int W, const int* pad, float* out, void* stream) {
  if (!x || !out || !pad || NC < 1 || T < 1 || H < 1 || W < 1 || pad[0] < 0 || pad[1] < 0 || pad[2] < 0) return HPVG_ERR_ARG;
  const double dT = (double)T + 2.0 * pad[0], dH = (double)H + 2.0 * pad[1], dW = (double)W + 2.0 * pad[2];
  if ((double)NC * dT * dH * dW >= 2147483648.0) return HPVG_ERR_UNSUPPORTED;
  RingPadGeom g;
  g.T = T; g.H = H; g.W = W;
  g.dT = (int)dT; g.dH = (int)dH; g.dW = (int)dW;
  g.t0 = ring_mod(-(long)pad[0], T);
  g.h0 = ring_mod(-(long)pad[1], H);
  g.w0 = ring_mod(-(long)pad[2], W);
  const long n = NC * g.dT * g.dH * g.dW;
  // a gather: other threads read x while out is written
  const uintptr_t s0 = (uintptr_t)x, s1 = s0 + (size_t)NC * T * H * W * sizeof(float);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)n * sizeof(float);
  if (o0 < s1 && s0 < o1) return HPVG_ERR_ARG;
  if (o0 & 3) return HPVG_ERR_ARG;
  long head = (long)(((16 - (o0 & 15)) & 15) >> 2);
  if (head > n) head = n;
  const long nvec = (n - head) / 4;
  long nb = (nvec + 2 + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(ring_pad_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, out, n, (int)head, nvec, g);
  return hpvg_launch_status();
}

int hpvg_upsample_linear_ring_f32(const float* x, long NC, int Ts, int Hs, int Ws, float* out, int To, int Ho, int Wo, const int* wrap,
                                  void* stream) {
  if (!x || !out || NC < 1 || Ts < 1 || Hs < 1 || Ws < 1 || To < 1 || Ho < 1 || Wo < 1) return HPVG_ERR_ARG;
  int rings = 0;
  if (wrap) {
    for (int a = 0; a < 3; ++a) {
      if (wrap[a] != 0 && wrap[a] != 1) return HPVG_ERR_ARG;
      rings |= wrap[a] << a;
    }
  }
  const long n = NC * To * Ho * Wo;
  if (!rings)   // the align-corners resize itself: the same kernel, the same bits
    hipLaunchKernelGGL(upsample_fwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, out, (const float*)nullptr, 0.f,
                       (float*)nullptr, NC, Ts, Hs, Ws, To, Ho, Wo, ac_scale(Ts, To), ac_scale(Hs, Ho), ac_scale(Ws, Wo));
  else
    hipLaunchKernelGGL(upsample_ring_fwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, out, NC, Ts, Hs, Ws, To, Ho,
                       Wo, ac_scale(Ts, To), ac_scale(Hs, Ho), ac_scale(Ws, Wo), rings);
  return hpvg_launch_status();
}

}  // extern "C"
