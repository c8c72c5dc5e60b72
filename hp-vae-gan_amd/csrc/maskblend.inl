// Dilate-and-feather composite of two uint8 volumes (generate --guide-mask, generate_patchnn --guide-mask): the contract written
// out at hpvg_mask_blend_u8 in hpvg.h; this file is one way to compute it.
//
// dil = the box maximum of (mask != 0) and c = the box sum of dil are both separable, so the work is at most six 1-D passes, a
// thread per voxel, each a gather of up to 2 r + 1 neighbours along one axis, clipped at the borders:
//   max along x, y, t   uint8 -> uint8    (two byte planes of the workspace, ping-pong; the first reads the mask itself)
//   sum along x, y      uint8 / uint16 -> uint16   (two uint16 planes; a sum along two axes is at most 129^2 < 2^16)
//   sum along t, n(v) from the clipped box sides, and the blend (2 (c a + (n - c) b) + n) / (2 n) per channel, in one kernel
// A pass whose radius is 0 is the identity and is not launched: radius (0, 0, 0) is the last kernel alone, reading the mask.
// Every pass reads one plane and writes another, all sums are integers: no atomics, no host synchronisation, and the result is
// a function of the arguments alone.
namespace {

constexpr int MB_MAX_RADIUS = 64;
constexpr int MB_THREADS = 256;

struct MbGeom {
  int T, H, W;
  long V;
};

// the coordinate of voxel i along `axis` (0 t, 1 y, 2 x), that axis' side and the element stride along it
__device__ inline void mb_axis(const MbGeom& g, long i, int axis, int& p, int& L, long& stride) {
  if (axis == 2) { p = (int)(i % g.W); L = g.W; stride = 1; }
  else if (axis == 1) { p = (int)((i / g.W) % g.H); L = g.H; stride = g.W; }
  else { p = (int)(i / ((long)g.W * g.H)); L = g.T; stride = (long)g.W * g.H; }
}

__global__ __launch_bounds__(MB_THREADS) void mb_max_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                             MbGeom g, int axis, int r) {
  for (long i = (long)blockIdx.x * MB_THREADS + threadIdx.x; i < g.V; i += (long)gridDim.x * MB_THREADS) {
    int p, L;
    long s;
    mb_axis(g, i, axis, p, L, s);
    const int lo = p - r < 0 ? 0 : p - r, hi = p + r > L - 1 ? L - 1 : p + r;
    const unsigned char* q = src + (i - (long)p * s);
    unsigned char m = 0;
    for (int k = lo; k <= hi; ++k) m |= (unsigned char)(q[k * s] != 0);
    dst[i] = m;
  }
}

template <typename In>
__global__ __launch_bounds__(MB_THREADS) void mb_sum_kernel(const In* __restrict__ src, unsigned short* __restrict__ dst, MbGeom g,
                                                             int axis, int r) {
  for (long i = (long)blockIdx.x * MB_THREADS + threadIdx.x; i < g.V; i += (long)gridDim.x * MB_THREADS) {
    int p, L;
    long s;
    mb_axis(g, i, axis, p, L, s);
    const int lo = p - r < 0 ? 0 : p - r, hi = p + r > L - 1 ? L - 1 : p + r;
    const In* q = src + (i - (long)p * s);
    unsigned acc = 0;
    for (int k = lo; k <= hi; ++k) {
      const unsigned v = q[k * s];
      acc += std::is_same<In, unsigned char>::value ? (unsigned)(v != 0) : v;
    }
    dst[i] = (unsigned short)acc;
  }
}

__device__ inline int mb_side(int p, int L, int r) {
  const int lo = p - r < 0 ? 0 : p - r, hi = p + r > L - 1 ? L - 1 : p + r;
  return hi - lo + 1;
}

// the sum along t of the counts so far (In = uint8: 0 / nonzero flags; uint16: sums along x and y), n from the box, the blend
template <typename In>
__global__ __launch_bounds__(MB_THREADS) void mb_blend_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                               const In* __restrict__ cnt, unsigned char* __restrict__ out, MbGeom g,
                                                               int rt, int rh, int rw) {
  const long plane = (long)g.W * g.H;
  for (long i = (long)blockIdx.x * MB_THREADS + threadIdx.x; i < g.V; i += (long)gridDim.x * MB_THREADS) {
    const int x = (int)(i % g.W), y = (int)((i / g.W) % g.H), t = (int)(i / plane);
    const int lo = t - rt < 0 ? 0 : t - rt, hi = t + rt > g.T - 1 ? g.T - 1 : t + rt;
    const In* q = cnt + (i - (long)t * plane);
    unsigned c = 0;
    for (int k = lo; k <= hi; ++k) {
      const unsigned v = q[k * plane];
      c += std::is_same<In, unsigned char>::value ? (unsigned)(v != 0) : v;
    }
    const unsigned n = (unsigned)(hi - lo + 1) * (unsigned)mb_side(y, g.H, rh) * (unsigned)mb_side(x, g.W, rw);
    const unsigned char* pa = a + i * 3;
    const unsigned char* pb = b + i * 3;
    unsigned char* po = out + i * 3;
    // 2 (c a + (n - c) b) + n <= 511 n <= 511 * 129^3 < 2^31
    for (int ch = 0; ch < 3; ++ch) po[ch] = (unsigned char)((2u * (c * pa[ch] + (n - c) * pb[ch]) + n) / (2u * n));
  }
}

inline size_t mb_up16(size_t n) { return (n + 15) & ~(size_t)15; }

// HPVG_OK and the geometry, or the refusal of the sides and radii
inline int mb_geom(MbGeom& g, int T, int H, int W, const int* radius) {
  if (T < 1 || H < 1 || W < 1 || !radius) return HPVG_ERR_ARG;
  for (int k = 0; k < 3; ++k)
    if (radius[k] < 0 || radius[k] > MB_MAX_RADIUS) return HPVG_ERR_ARG;
  if ((double)T * (double)H * (double)W >= 2147483648.0) return HPVG_ERR_UNSUPPORTED;
  g.T = T; g.H = H; g.W = W;
  g.V = (long)T * H * W;
  return HPVG_OK;
}

inline size_t mb_ws_bytes(const MbGeom& g, const int* radius) {
  if (!(radius[0] | radius[1] | radius[2])) return 0;
  return 2 * mb_up16((size_t)g.V) + 2 * mb_up16(2 * (size_t)g.V);   // two byte planes and two uint16 planes
}

inline bool mb_overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return p0 < q0 + nq && q0 < p0 + np;
}

}  // namespace

extern "C" {

size_t hpvg_mask_blend_ws_bytes(int T, int H, int W, const int* radius) {
  MbGeom g;
  if (mb_geom(g, T, H, W, radius) != HPVG_OK) return 0;
  return mb_ws_bytes(g, radius);
}

int hpvg_mask_blend_u8(const unsigned char* a, const unsigned char* b, const unsigned char* mask, int T, int H, int W,
                       const int* radius, unsigned char* out, void* ws, size_t ws_bytes, void* stream) {
  MbGeom g;
  const int rc = mb_geom(g, T, H, W, radius);
  if (rc != HPVG_OK) return rc;
  if (!a || !b || !mask || !out) return HPVG_ERR_ARG;
  const size_t V = (size_t)g.V;
  // gathers: other threads read the inputs while out is written
  if (mb_overlap(out, 3 * V, a, 3 * V) || mb_overlap(out, 3 * V, b, 3 * V) || mb_overlap(out, 3 * V, mask, V)) return HPVG_ERR_ARG;
  const size_t need = mb_ws_bytes(g, radius);
  if (need && (!ws || ((uintptr_t)ws & 15) || ws_bytes < need)) return HPVG_ERR_WORKSPACE;
  const int rt = radius[0], rh = radius[1], rw = radius[2];
  hipStream_t st = (hipStream_t)stream;
  long nb = (g.V + MB_THREADS - 1) / MB_THREADS;
  if (nb > 65536) nb = 65536;
  const dim3 grid((unsigned)nb), block(MB_THREADS);

  unsigned char* byte_plane[2] = {(unsigned char*)ws, (unsigned char*)ws + mb_up16(V)};
  unsigned short* word_plane[2] = {(unsigned short*)((unsigned char*)ws + 2 * mb_up16(V)),
                                   (unsigned short*)((unsigned char*)ws + 2 * mb_up16(V) + mb_up16(2 * V))};
  // dilation: x, y, t
  const unsigned char* flags = mask;
  int next = 0;
  const int axes[3] = {2, 1, 0}, rad[3] = {rw, rh, rt};
  for (int k = 0; k < 3; ++k) {
    if (!rad[k]) continue;
    hipLaunchKernelGGL(mb_max_kernel, grid, block, 0, st, flags, byte_plane[next], g, axes[k], rad[k]);
    flags = byte_plane[next];
    next ^= 1;
  }
  // box count: x, y through the uint16 planes, t inside the blend
  const unsigned short* sums = nullptr;
  if (rw) {
    hipLaunchKernelGGL(mb_sum_kernel<unsigned char>, grid, block, 0, st, flags, word_plane[0], g, 2, rw);
    sums = word_plane[0];
  }
  if (rh) {
    if (sums) {
      hipLaunchKernelGGL(mb_sum_kernel<unsigned short>, grid, block, 0, st, sums, word_plane[1], g, 1, rh);
      sums = word_plane[1];
    } else {
      hipLaunchKernelGGL(mb_sum_kernel<unsigned char>, grid, block, 0, st, flags, word_plane[0], g, 1, rh);
      sums = word_plane[0];
    }
  }
  if (sums)
    hipLaunchKernelGGL(mb_blend_kernel<unsigned short>, grid, block, 0, st, a, b, sums, out, g, rt, rh, rw);
  else
    hipLaunchKernelGGL(mb_blend_kernel<unsigned char>, grid, block, 0, st, a, b, flags, out, g, rt, rh, rw);
  return hpvg_launch_status();
}

}  // extern "C"
