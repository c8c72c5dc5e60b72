// Deterministic PatchMatch (generate_patchnn --search patchmatch): an approximate nearest-neighbour field between the dense
// patch grids of two uint8 volumes whose cost is linear in the number of patches.  The rule - hash start, Jacobi iterations of
// six propagation candidates and a shrinking random search, keys (d2, j) or (float32(d2) * w_j, j) compared lexicographically -
// is the contract written out at hpvg_patchmatch_u8 in hpvg.h; this file is one way to compute it.
//
// One kernel, one launch per iteration (and one for the start): patchmatch_kernel reads the field of the previous launch and
// writes the next one, so no thread ever sees a value of its own launch (Jacobi) and the result cannot depend on scheduling.
// The two fields live in the workspace; the last launch writes the outputs.  Nothing is synchronised with the host.
//
// Shape: one thread per query patch, a workgroup per 8 x 32 tile of the query grid at one t.  A thread scores at most
// 6 + 16 candidates of D bytes each, and the candidates of neighbouring threads are mostly neighbouring key patches, so the key
// bytes come from the cache (the key volume is a few MB); the tile's own query voxels - pt x (8 + ph - 1) x (32 + pw - 1) x 3
// bytes - are staged in LDS once and every candidate re-reads them from there.  A patch line is pw * 3 contiguous bytes at a
// byte offset of any alignment: the LDS side reads aligned words and shifts neighbouring pairs (v_alignbyte_b32), the key side
// reads unaligned words straight from global memory, and four byte pairs at a time go through v_dot4_u32_u8 as
// sum a^2 + sum b^2 - 2 sum ab (unsigned, exact: 2 D 255^2 < 2^32).  The partial sum after a line is the exact distance of the
// lines so far, so a candidate stops at the first line after which it can no longer win; with weights the test is on
// float32(partial) * w, which is monotone in partial for w > 0.  Neither changes a result.
// A patch too large for 64 KB of LDS (very long pt) takes the same kernel with the query read from global memory.
namespace {

constexpr int PM_TX = 32, PM_TY = 8;      // the workgroup's tile of the query grid: 8 rows of 32 patches
constexpr size_t PM_LDS_MAX = 65536;

struct PmGeom {
  int Hq, Wq, Hr, Wr;
  int gT, gH, gW, kT, kH, kW;   // query grid, key grid
  int pt, ph, pw;
  int run, nw, tail;            // bytes of a patch line, its whole words, the bytes after them
  int lrow, lrows;              // LDS: bytes between two rows (a multiple of 4), rows per plane
  int R;                        // the first radius of the random search: the key grid's largest side
  long Nq, Nr;
  size_t lds;                   // bytes of LDS for the tile, 0: the query is read from global memory
  size_t off_field[2], bytes;   // the two fields in the workspace
};

struct PmField {   // [Nq] each
  int* nn;
  int* d2;
  float* score;
};

inline bool pm_geom(PmGeom& g, int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch) {
  PnnGeom p;
  const int one[3] = {1, 1, 1};
  if (!pnn_geom(p, Tq, Hq, Wq, Tr, Hr, Wr, patch, one, one)) return false;
  const int sides[6] = {p.q.nT, p.q.nY, p.q.nX, p.r.nT, p.r.nY, p.r.nX};
  for (int k = 0; k < 6; ++k)
    if (sides[k] >= 65536) return false;
  g.Hq = Hq; g.Wq = Wq; g.Hr = Hr; g.Wr = Wr;
  g.gT = p.q.nT; g.gH = p.q.nY; g.gW = p.q.nX;
  g.kT = p.r.nT; g.kH = p.r.nY; g.kW = p.r.nX;
  g.pt = p.p.pt; g.ph = p.p.ph; g.pw = p.p.pw;
  g.run = 3 * g.pw; g.nw = g.run >> 2; g.tail = g.run & 3;
  g.lrow = ((PM_TX + g.pw - 1) * 3 + 3) & ~3;
  g.lrows = PM_TY + g.ph - 1;
  g.R = g.kT > g.kH ? g.kT : g.kH;
  if (g.kW > g.R) g.R = g.kW;
  g.Nq = p.q.N; g.Nr = p.r.N;
  const double lds = (double)g.pt * g.lrows * g.lrow + 8;   // + 8: the shifted reads look one word past a line's end
  g.lds = lds <= (double)PM_LDS_MAX ? (size_t)lds : 0;
  size_t o = 0;
  for (int f = 0; f < 2; ++f) {
    g.off_field[f] = o;
    o = pnn_align(o + 3 * pnn_align((size_t)g.Nq * 4));
  }
  g.bytes = o;
  return true;
}

__device__ __forceinline__ unsigned pm_h32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ unsigned pm_rnd(unsigned seed, unsigned i, unsigned it, unsigned k, unsigned ax) {
  return pm_h32(seed + i * 0x9E3779B9u + (it * 64u + k * 4u + ax) * 0x85EBCA6Bu);
}

__device__ __forceinline__ int pm_mod(int c, int side) {   // the non-negative modulus
  c %= side;
  return c < 0 ? c + side : c;
}

__device__ __forceinline__ unsigned pm_load4(const unsigned char* p) {   // any alignment
  unsigned v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

__device__ __forceinline__ unsigned pm_load_tail(const unsigned char* p, int n) {   // n = 1 .. 3 bytes, nothing past them
  unsigned v = p[0];
  if (n > 1) v |= (unsigned)p[1] << 8;
  if (n > 2) v |= (unsigned)p[2] << 16;
  return v;
}

// the running best of one query patch: its key, and the key coordinate
template <bool WEIGHTED>
struct PmBest {
  int d2, j, t, y, x;
  float sc;
  __device__ __forceinline__ bool beaten_by(int cd2, float csc, int cj) const {
    if constexpr (WEIGHTED) return csc < sc || (csc == sc && cj < j);
    else return cd2 < d2 || (cd2 == d2 && cj < j);
  }
};

// The exact squared distance between the thread's query patch and the key patch at (ct, cy, cx), or -1 as soon as the lines
// summed so far show that the candidate's key is larger than the running best's.  QLDS: qp is the patch's first byte in the
// LDS tile (rows lrow apart, planes lrows rows apart); otherwise in the query volume.
template <bool WEIGHTED, bool QLDS>
__device__ __forceinline__ int pm_distance(const PmGeom& g, const unsigned char* qp, const unsigned char* __restrict__ r, int ct, int cy,
                                           int cx, bool bounded, int bound_d2, float bound_sc, float w) {
  unsigned pos = 0, cross = 0;   // sum a^2 + sum b^2, sum ab
  const long qrow = QLDS ? g.lrow : (long)g.Wq * 3, qplane = QLDS ? (long)g.lrows * g.lrow : (long)g.Hq * g.Wq * 3;
  const unsigned tmask = (1u << (8 * g.tail)) - 1u;
  for (int dt = 0; dt < g.pt; ++dt) {
    const unsigned char* kl = r + (((long)(ct + dt) * g.Hr + cy) * g.Wr + cx) * 3;
    const unsigned char* ql = qp + dt * qplane;
    for (int dy = 0; dy < g.ph; ++dy, kl += (long)g.Wr * 3, ql += qrow) {
      if constexpr (QLDS) {
        const unsigned sh = (unsigned)((uintptr_t)ql & 3);
        const unsigned* qw = (const unsigned*)(ql - sh);
        unsigned lo = qw[0];
        for (int k = 0; k < g.nw; ++k) {
          const unsigned hi = qw[k + 1];
          const unsigned a = __builtin_amdgcn_alignbyte(hi, lo, sh), b = pm_load4(kl + 4 * k);
          lo = hi;
          pos = __builtin_amdgcn_udot4(a, a, pos, false);
          pos = __builtin_amdgcn_udot4(b, b, pos, false);
          cross = __builtin_amdgcn_udot4(a, b, cross, false);
        }
        if (g.tail) {
          const unsigned a = __builtin_amdgcn_alignbyte(qw[g.nw + 1], lo, sh) & tmask, b = pm_load_tail(kl + 4 * g.nw, g.tail);
          pos = __builtin_amdgcn_udot4(a, a, pos, false);
          pos = __builtin_amdgcn_udot4(b, b, pos, false);
          cross = __builtin_amdgcn_udot4(a, b, cross, false);
        }
      } else {
        for (int k = 0; k < g.nw; ++k) {
          const unsigned a = pm_load4(ql + 4 * k), b = pm_load4(kl + 4 * k);
          pos = __builtin_amdgcn_udot4(a, a, pos, false);
          pos = __builtin_amdgcn_udot4(b, b, pos, false);
          cross = __builtin_amdgcn_udot4(a, b, cross, false);
        }
        if (g.tail) {
          const unsigned a = pm_load_tail(ql + 4 * g.nw, g.tail), b = pm_load_tail(kl + 4 * g.nw, g.tail);
          pos = __builtin_amdgcn_udot4(a, a, pos, false);
          pos = __builtin_amdgcn_udot4(b, b, pos, false);
          cross = __builtin_amdgcn_udot4(a, b, cross, false);
        }
      }
      if (bounded) {
        const int part = (int)(pos - 2u * cross);
        if constexpr (WEIGHTED) {
          if (__fmul_rn((float)part, w) > bound_sc) return -1;
        } else {
          if (part > bound_d2) return -1;
        }
      }
    }
  }
  return (int)(pos - 2u * cross);
}

// One candidate against the running best.  A candidate that IS the running best has the same key and cannot replace it.
template <bool WEIGHTED, bool QLDS>
__device__ __forceinline__ void pm_try(const PmGeom& g, const unsigned char* qp, const unsigned char* __restrict__ r,
                                       const float* __restrict__ rw, PmBest<WEIGHTED>& best, int ct, int cy, int cx) {
  const int cj = (ct * g.kH + cy) * g.kW + cx;
  if (cj == best.j) return;
  float w = 1.0f;
  if constexpr (WEIGHTED) w = rw[cj];
  const int d = pm_distance<WEIGHTED, QLDS>(g, qp, r, ct, cy, cx, true, best.d2, best.sc, w);
  if (d < 0) return;
  float sc = 0.0f;
  if constexpr (WEIGHTED) sc = __fmul_rn((float)d, w);
  if (best.beaten_by(d, sc, cj)) {
    best.d2 = d; best.sc = sc; best.j = cj;
    best.t = ct; best.y = cy; best.x = cx;
  }
}

// grid: (ceil(gW / 32), ceil(gH / 8), gT); thread (tx, ty) of a workgroup owns one query patch.  start: the launch that scores
// the start (nn_init clamped, or the hash start) and reads no field; otherwise iteration `it` from src to dst.
// WRAP (hpvg_patchmatch_wrap_u8): bit ax of qwm / rwm says that axis ax of the query / key grid is a ring; the volumes arrive
// circularly padded, so everything but the neighbourhood rule is the same code.  Without WRAP the masks are not read.
template <bool WEIGHTED, bool QLDS, bool WRAP>
__global__ __launch_bounds__(PM_TX * PM_TY) void patchmatch_kernel(const unsigned char* __restrict__ q, const unsigned char* __restrict__ r,
                                                                    const float* __restrict__ rw, const int* __restrict__ nn_init,
                                                                    PmField src, PmField dst, PmGeom g, unsigned seed, int it,
                                                                    int start, int qwm, int rwm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pm_lds[];
  const int tx = threadIdx.x & (PM_TX - 1), ty = threadIdx.x / PM_TX;
  const int ax0 = blockIdx.x * PM_TX, ay0 = blockIdx.y * PM_TY, at = blockIdx.z;
  const int ax = ax0 + tx, ay = ay0 + ty;
  const unsigned char* qp;
  if constexpr (QLDS) {
    // the tile's voxels, clipped to the volume: rows ay0 .. ay0 + lrows - 1, bytes 3 ax0 .. 3 (ax0 + 32 + pw - 1) - 1
    const int rows = min(g.lrows, g.Hq - ay0), bytes = min((PM_TX + g.pw - 1) * 3, (g.Wq - ax0) * 3);
    const int total = g.pt * rows * bytes;
    for (int e = threadIdx.x; e < total; e += PM_TX * PM_TY) {
      const int b = e % bytes, row = (e / bytes) % rows, pl = e / (bytes * rows);
      pm_lds[(pl * g.lrows + row) * g.lrow + b] = q[(((long)(at + pl) * g.Hq + ay0 + row) * g.Wq + ax0) * 3 + b];
    }
    __syncthreads();
    qp = pm_lds + ty * g.lrow + tx * 3;
  } else {
    qp = q + (((long)at * g.Hq + ay) * g.Wq + ax) * 3;
  }
  if (ax >= g.gW || ay >= g.gH) return;
  const int i = (at * g.gH + ay) * g.gW + ax;

  PmBest<WEIGHTED> best;
  if (start) {
    if (nn_init) {
      long j = nn_init[i];
      j = j < 0 ? 0 : (j >= g.Nr ? g.Nr - 1 : j);
      best.j = (int)j;
      best.x = best.j % g.kW; best.y = (best.j / g.kW) % g.kH; best.t = best.j / (g.kW * g.kH);
    } else {
      best.t = (int)(pm_rnd(seed, (unsigned)i, 0xFFFFFFu, 0u, 0u) % (unsigned)g.kT);
      best.y = (int)(pm_rnd(seed, (unsigned)i, 0xFFFFFFu, 0u, 1u) % (unsigned)g.kH);
      best.x = (int)(pm_rnd(seed, (unsigned)i, 0xFFFFFFu, 0u, 2u) % (unsigned)g.kW);
      best.j = (best.t * g.kH + best.y) * g.kW + best.x;
    }
    best.d2 = pm_distance<WEIGHTED, QLDS>(g, qp, r, best.t, best.y, best.x, false, 0, 0.0f, 1.0f);
    best.sc = 0.0f;
    if constexpr (WEIGHTED) best.sc = __fmul_rn((float)best.d2, rw[best.j]);
  } else {
    // the patch's own old match, then the six neighbours' old matches, shifted back
    long j = src.nn[i];
    j = j < 0 ? 0 : (j >= g.Nr ? g.Nr - 1 : j);   // (a field of this call is always in range)
    best.j = (int)j;
    best.x = best.j % g.kW; best.y = (best.j / g.kW) % g.kH; best.t = best.j / (g.kW * g.kH);
    best.d2 = src.d2[i];
    best.sc = 0.0f;
    if constexpr (WEIGHTED) best.sc = src.score[i];
    const int a[3] = {at, ay, ax}, gs[3] = {g.gT, g.gH, g.gW}, ks[3] = {g.kT, g.kH, g.kW};
    const int stride[3] = {g.gH * g.gW, g.gW, 1};
#pragma unroll
    for (int axis = 0; axis < 3; ++axis)
#pragma unroll
      for (int s = -1; s <= 1; s += 2) {
        int na = a[axis] + s;
        if (WRAP && ((qwm >> axis) & 1)) na = na < 0 ? gs[axis] - 1 : (na >= gs[axis] ? 0 : na);
        else if (na < 0 || na >= gs[axis]) continue;
        long nj = src.nn[i + (na - a[axis]) * stride[axis]];
        nj = nj < 0 ? 0 : (nj >= g.Nr ? g.Nr - 1 : nj);
        int c[3] = {(int)(nj / (g.kW * g.kH)), (int)((nj / g.kW) % g.kH), (int)(nj % g.kW)};
        c[axis] -= s;
        if (WRAP && ((rwm >> axis) & 1)) c[axis] = c[axis] < 0 ? ks[axis] - 1 : (c[axis] >= ks[axis] ? 0 : c[axis]);
        else if (c[axis] < 0 || c[axis] >= ks[axis]) continue;
        pm_try<WEIGHTED, QLDS>(g, qp, r, rw, best, c[0], c[1], c[2]);
      }
    // the random search around the running best, radius R, R / 2, ... 1
    for (int k = 0; (g.R >> k) >= 1; ++k) {
      const int rk = g.R >> k;
      const unsigned span = 2u * (unsigned)rk + 1u;
      int ct = best.t + (int)(pm_rnd(seed, (unsigned)i, (unsigned)it, (unsigned)k, 0u) % span) - rk;
      int cy = best.y + (int)(pm_rnd(seed, (unsigned)i, (unsigned)it, (unsigned)k, 1u) % span) - rk;
      int cx = best.x + (int)(pm_rnd(seed, (unsigned)i, (unsigned)it, (unsigned)k, 2u) % span) - rk;
      if (WRAP && (rwm & 1)) ct = pm_mod(ct, g.kT);
      else ct = ct < 0 ? 0 : (ct >= g.kT ? g.kT - 1 : ct);
      if (WRAP && (rwm & 2)) cy = pm_mod(cy, g.kH);
      else cy = cy < 0 ? 0 : (cy >= g.kH ? g.kH - 1 : cy);
      if (WRAP && (rwm & 4)) cx = pm_mod(cx, g.kW);
      else cx = cx < 0 ? 0 : (cx >= g.kW ? g.kW - 1 : cx);
      pm_try<WEIGHTED, QLDS>(g, qp, r, rw, best, ct, cy, cx);
    }
  }
  dst.nn[i] = best.j;
  dst.d2[i] = best.d2;
  if constexpr (WEIGHTED)
    if (dst.score) dst.score[i] = best.sc;
}

template <bool WEIGHTED, bool WRAP>
void pm_launch_one(const PmGeom& g, const unsigned char* q, const unsigned char* r, const float* rw, const int* nn_init, PmField src,
                   PmField dst, unsigned seed, int it, int start, int qwm, int rwm, hipStream_t st) {
  const dim3 grid((unsigned)((g.gW + PM_TX - 1) / PM_TX), (unsigned)((g.gH + PM_TY - 1) / PM_TY), (unsigned)g.gT);
  if (g.lds)
    hipLaunchKernelGGL((patchmatch_kernel<WEIGHTED, true, WRAP>), grid, dim3(PM_TX * PM_TY), g.lds, st, q, r, rw, nn_init, src, dst, g,
                       seed, it, start, qwm, rwm);
  else
    hipLaunchKernelGGL((patchmatch_kernel<WEIGHTED, false, WRAP>), grid, dim3(PM_TX * PM_TY), 0, st, q, r, rw, nn_init, src, dst, g,
                       seed, it, start, qwm, rwm);
}

// ring flags as a bit mask (bit ax = axis ax); null: 0; -1 for an entry other than 0 / 1
inline int pm_wrap_mask(const int* wrap) {
  int m = 0;
  for (int ax = 0; wrap && ax < 3; ++ax) {
    if (wrap[ax] != 0 && wrap[ax] != 1) return -1;
    m |= wrap[ax] << ax;
  }
  return m;
}

// both entry points: the refusals, the two fields in the workspace, one launch for the start and one per iteration
int pm_run(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr, const int* patch, int qwm,
           int rwm, const float* rweight, const int* nn_init, int iters, long seed, int* d2, int* nn, float* score, void* ws,
           size_t ws_bytes, void* stream) {
  PmGeom g;
  if (!q || !r || !d2 || !nn || (score && !rweight) || iters < 0 || iters > 1024 || qwm < 0 || rwm < 0 ||
      !pm_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch))
    return HPVG_ERR_ARG;
  if (!ws || ws_bytes < g.bytes || ((uintptr_t)ws & 15)) return HPVG_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const size_t part = pnn_align((size_t)g.Nq * 4);
  PmField f[2], out = {nn, d2, score};
  for (int k = 0; k < 2; ++k) {
    char* base = (char*)ws + g.off_field[k];
    f[k].nn = (int*)base;
    f[k].d2 = (int*)(base + part);
    f[k].score = (float*)(base + 2 * part);
  }
  const unsigned s32 = (unsigned)(unsigned long)seed;
  const bool wrap = (qwm | rwm) != 0;
  // launch 0 scores the start, launch 1 + it is iteration it; launch n writes field n & 1, the last one the outputs
  for (int n = 0; n <= iters; ++n) {
    const PmField src = f[(n + 1) & 1], dst = n == iters ? out : f[n & 1];
    if (wrap) {
      if (rweight) pm_launch_one<true, true>(g, q, r, rweight, nn_init, src, dst, s32, n - 1, n == 0, qwm, rwm, st);
      else pm_launch_one<false, true>(g, q, r, rweight, nn_init, src, dst, s32, n - 1, n == 0, qwm, rwm, st);
    } else {
      if (rweight) pm_launch_one<true, false>(g, q, r, rweight, nn_init, src, dst, s32, n - 1, n == 0, 0, 0, st);
      else pm_launch_one<false, false>(g, q, r, rweight, nn_init, src, dst, s32, n - 1, n == 0, 0, 0, st);
    }
  }
  return hpvg_launch_status();
}

}  // namespace

extern "C" {

size_t hpvg_patchmatch_ws_bytes(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch) {
  PmGeom g;
  if (!pm_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch)) return 0;
  return g.bytes;
}

int hpvg_patchmatch_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr, const int* patch,
                       const float* rweight, const int* nn_init, int iters, long seed, int* d2, int* nn, float* score, void* ws,
                       size_t ws_bytes, void* stream) {
  return pm_run(q, Tq, Hq, Wq, r, Tr, Hr, Wr, patch, 0, 0, rweight, nn_init, iters, seed, d2, nn, score, ws, ws_bytes, stream);
}

int hpvg_patchmatch_wrap_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr,
                            const int* patch, const int* qwrap, const int* rwrap, const float* rweight, const int* nn_init, int iters,
                            long seed, int* d2, int* nn, float* score, void* ws, size_t ws_bytes, void* stream) {
  return pm_run(q, Tq, Hq, Wq, r, Tr, Hr, Wr, patch, pm_wrap_mask(qwrap), pm_wrap_mask(rwrap), rweight, nn_init, iters, seed, d2, nn,
                score, ws, ws_bytes, stream);
}

}  // extern "C"
