// Exact antialiased resize of a uint8 volume [Ts][Hs][Ws][3] to [To][Ho][Wo][3] (generate_patchnn --antialias / --t-ratio,
// evaluate --scales): the contract written out at hpvg_volume_resize_u8 in hpvg.h; this file is one way to compute it.
//
// Per axis of S source and O output positions the integer weight of source i for output o is
// w = max(0, R - |i (O - 1) - o (S - 1)|), R = max(O - 1, S - 1) (S == O: the identity), so the sources with w > 0 are the run
// [lo, hi) of VrAxis below, and an output voxel is (2 N + D) / (2 D) with N = sum wt wh ww v and D = sum wt wh ww over the
// box of the three runs.  Both sums are 64-bit integer additions: associative and commutative, so however the box is split
// between lanes the result is the same, and the host has checked 511 D < 2^63 before the launch.
//
// A gather, two shapes of one kernel (volresize_kernel<G>): G lanes walk the flattened box of one output voxel with stride G
// (x fastest, so neighbouring lanes read neighbouring voxels), each with its own partial N (3 channels) and D, and for G = 64
// the wave adds them by xor shuffles.  G = 1 - a thread per output voxel - serves the pyramid's ordinary steps, whose boxes hold
// 8 (upsizing) to a few dozen voxels; G = 64 - a wave per output voxel - serves the coarse levels made from the full-size
// volume, with few outputs and boxes of hundreds to thousands of voxels (the host picks it when the largest box has at least
// VR_WAVE_BOX voxels).  No workspace, no atomics, one launch.
namespace {

constexpr long VR_WAVE_BOX = 64;   // the largest box, in voxels, from which a wave takes one output voxel

struct VrAxis {
  long a, c, R;   // w(o, i) = R - |i a - o c|: a = O - 1, c = S - 1 (identity axis: a = c = 0 and R = 1, the run is {o})
  int S, O, same;
};

struct VrGeom {
  VrAxis t, h, w;
};

inline VrAxis vr_axis(int S, int O) {
  VrAxis x;
  x.S = S; x.O = O; x.same = S == O;
  x.a = x.same ? 0 : O - 1;
  x.c = x.same ? 0 : S - 1;
  x.R = x.same ? 1 : (O > S ? O - 1 : S - 1);
  return x;
}

// the run [lo, hi) of sources with a positive weight for output o: R - |i a - o c| > 0
__host__ __device__ inline void vr_run(const VrAxis& x, int o, int& lo, int& hi) {
  if (x.same) { lo = o; hi = o + 1; return; }
  if (x.a == 0) { lo = 0; hi = x.S; return; }   // one output: the whole axis, all weights R
  const long b = (long)o * x.c;
  // i a > b - R  and  i a < b + R
  const long l = b - x.R < 0 ? 0 : (b - x.R) / x.a + 1;
  const long h = (b + x.R + x.a - 1) / x.a;     // the smallest i with i a >= b + R
  lo = (int)l;
  hi = (int)(h > x.S ? x.S : h);
}

__host__ __device__ inline long vr_weight(const VrAxis& x, int o, int i) {
  const long d = (long)i * x.a - (long)o * x.c;
  return x.R - (d < 0 ? -d : d);
}

template <int G>
__global__ __launch_bounds__(256) void volresize_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ out,
                                                         VrGeom g) {
  const long total = (long)g.t.O * g.h.O * g.w.O;
  const int lane = G == 1 ? 0 : (int)(threadIdx.x & (G - 1));
  const long per_block = 256 / G;
  // every lane of a group runs the same number of trips (the shuffles below need the whole wave)
  for (long o = (long)blockIdx.x * per_block + threadIdx.x / G; o < total; o += (long)gridDim.x * per_block) {
    const int ox = (int)(o % g.w.O);
    const int oy = (int)((o / g.w.O) % g.h.O);
    const int ot = (int)(o / ((long)g.w.O * g.h.O));
    int t0, t1, y0, y1, x0, x1;
    vr_run(g.t, ot, t0, t1);
    vr_run(g.h, oy, y0, y1);
    vr_run(g.w, ox, x0, x1);
    unsigned long long n0 = 0, n1 = 0, n2 = 0, den = 0;
    if (G == 1) {
      for (int t = t0; t < t1; ++t) {
        const long wt = vr_weight(g.t, ot, t);
        for (int y = y0; y < y1; ++y) {
          const long wty = wt * vr_weight(g.h, oy, y);
          const unsigned char* row = src + ((long)t * g.h.S + y) * g.w.S * 3;
          for (int x = x0; x < x1; ++x) {
            const unsigned long long w = (unsigned long long)(wty * vr_weight(g.w, ox, x));
            n0 += w * row[x * 3L];
            n1 += w * row[x * 3L + 1];
            n2 += w * row[x * 3L + 2];
            den += w;
          }
        }
      }
    } else {
      const int nx = x1 - x0, ny = y1 - y0;
      const long box = (long)(t1 - t0) * ny * nx;
      for (long k = lane; k < box; k += G) {
        const int x = x0 + (int)(k % nx);
        const int y = y0 + (int)((k / nx) % ny);
        const int t = t0 + (int)(k / ((long)nx * ny));
        const unsigned long long w = (unsigned long long)(vr_weight(g.t, ot, t) * vr_weight(g.h, oy, y) * vr_weight(g.w, ox, x));
        const unsigned char* b = src + (((long)t * g.h.S + y) * g.w.S + x) * 3;
        n0 += w * b[0];
        n1 += w * b[1];
        n2 += w * b[2];
        den += w;
      }
      for (int m = G / 2; m >= 1; m >>= 1) {
        n0 += __shfl_xor(n0, m, 64);
        n1 += __shfl_xor(n1, m, 64);
        n2 += __shfl_xor(n2, m, 64);
        den += __shfl_xor(den, m, 64);
      }
    }
    if (lane == 0) {
      unsigned char* dst = out + o * 3;
      dst[0] = (unsigned char)((2 * n0 + den) / (2 * den));
      dst[1] = (unsigned char)((2 * n1 + den) / (2 * den));
      dst[2] = (unsigned char)((2 * n2 + den) / (2 * den));
    }
  }
}

// per axis the largest sum of weights and the longest run over the outputs; false when a sum passes 2^62
inline bool vr_axis_max(const VrAxis& x, unsigned long long& wmax, long& nmax) {
  wmax = 0; nmax = 0;
  for (int o = 0; o < x.O; ++o) {
    int lo, hi;
    vr_run(x, o, lo, hi);
    unsigned long long s = 0;
    if (x.same || x.a == 0) {
      s = (unsigned long long)x.R * (unsigned long long)(hi - lo);
    } else {
      for (int i = lo; i < hi; ++i) s += (unsigned long long)vr_weight(x, o, i);
    }
    if (s > wmax) wmax = s;
    if (hi - lo > nmax) nmax = hi - lo;
  }
  return wmax < (1ULL << 62);
}

// the refusals and the two maxima of a resize, shared by the check and the launch
inline int vr_geom(VrGeom& g, int Ts, int Hs, int Ws, int To, int Ho, int Wo, long* out2) {
  if (Ts < 1 || Hs < 1 || Ws < 1 || To < 1 || Ho < 1 || Wo < 1) return HPVG_ERR_ARG;
  // the voxel counts the patch entry points take: each volume below 2^31 voxels
  if ((double)Ts * (double)Hs * (double)Ws >= 2147483648.0 || (double)To * (double)Ho * (double)Wo >= 2147483648.0)
    return HPVG_ERR_UNSUPPORTED;
  g.t = vr_axis(Ts, To);
  g.h = vr_axis(Hs, Ho);
  g.w = vr_axis(Ws, Wo);
  unsigned long long w[3];
  long n[3];
  if (!vr_axis_max(g.t, w[0], n[0]) || !vr_axis_max(g.h, w[1], n[1]) || !vr_axis_max(g.w, w[2], n[2])) return HPVG_ERR_UNSUPPORTED;
  const unsigned __int128 lim = (unsigned __int128)1 << 63;
  const unsigned __int128 d01 = (unsigned __int128)w[0] * w[1];   // factors below 2^62: no product here passes 2^128
  if (d01 >= lim) return HPVG_ERR_UNSUPPORTED;
  const unsigned __int128 d = d01 * w[2];
  if (d * 511 >= lim) return HPVG_ERR_UNSUPPORTED;
  if (out2) {
    out2[0] = (long)d;
    out2[1] = n[0] * n[1] * n[2];
  }
  return HPVG_OK;
}

}  // namespace

extern "C" {

int hpvg_volume_resize_check(int Ts, int Hs, int Ws, int To, int Ho, int Wo, long* out2) {
  VrGeom g;
  return vr_geom(g, Ts, Hs, Ws, To, Ho, Wo, out2);
}

int hpvg_volume_resize_u8(const unsigned char* src, int Ts, int Hs, int Ws, unsigned char* out, int To, int Ho, int Wo, void* stream) {
  VrGeom g;
  long m[2];
  const int rc = vr_geom(g, Ts, Hs, Ws, To, Ho, Wo, m);
  if (rc != HPVG_OK) return rc;
  if (!src || !out) return HPVG_ERR_ARG;
  // a gather: other threads read src while out is written
  const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)Ts * Hs * Ws * 3;
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)To * Ho * Wo * 3;
  if (o0 < s1 && s0 < o1) return HPVG_ERR_ARG;
  const long total = (long)To * Ho * Wo;
  const bool wave = m[1] >= VR_WAVE_BOX;
  const long per_block = wave ? 4 : 256;
  long blocks = (total + per_block - 1) / per_block;
  if (blocks > 65536) blocks = 65536;
  if (wave)
    hipLaunchKernelGGL(volresize_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, out, g);
  else
    hipLaunchKernelGGL(volresize_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, out, g);
  return hpvg_launch_status();
}

}  // extern "C"
