// Exact patch nearest neighbours between two uint8 volumes (the evaluate program's hot path): for every space-time patch of a
// query volume, the smallest squared distance to any patch of a reference volume and the smallest index that attains it
// (bidirectional patch similarity, Simakov et al. 2008: coherence one way, completeness the other).
//
// Volumes are channels-last uint8 [T][H][W][3]; patch i of a volume is the pt x ph x pw x 3 block at the i-th position, in
// (t, y, x) raster order, of the grid with the side's stride.  D = 3 * pt * ph * pw bytes per patch.
//
// Three kernels:
//   1. patchnn_pack_kernel (once per side): the centred int8 patch matrix [N padded to 128][D padded to 64, zeros] with
//      value = byte - 128, and the int32 squared norm of every row.  The query side also presets its rows' merge keys.
//   2. patchnn_min_kernel: an NT GEMM on v_mfma_i32_32x32x32_i8 (int32 accumulation) whose epilogue never stores the
//      Nq x Nr products: d2 = |q|^2 + |r|^2 - 2 q.r is exact in int32 as long as D * 255^2 < 2^31 (the centring shifts both
//      operands alike, so the distance is unchanged), each lane keeps a running (min, index) for its rows over the column tiles
//      its workgroup walks, the 32 lanes of a row merge once at the end and the row's winner goes into a 64-bit key
//      (d2 << 32) | j with a vector global atomic umin.  min is associative and commutative and the index rides in the low
//      bits, so the result is independent of the launch geometry and of timing, and ties resolve to the smallest index.
//   3. patchnn_unpack_kernel: key -> d2, nn.
//
// Subset search (the patch inpainting of generate_patchnn --mask: only the patches that overlap the hole are queries, only the
// patches that avoid it are keys): either side may bring an ascending int32 list of grid indices.  The pack gathers only the
// listed patches (row i of the matrix is grid patch sel[i], clamped into the grid, so nothing outside a volume is ever read),
// kernel 2 runs unchanged on the compacted matrices, whose sizes - and the workspace - follow the lists' lengths, and
// patchnn_unpack_subset_kernel scatters row i's key to d2 / nn [qsel[i]] with the winner translated back through rsel, after
// patchnn_fill_kernel has written -1 to every entry of the full-grid outputs.  Compacted rows keep the lists' order, so the
// smallest compacted index among equals is the smallest grid index.
//
// Mask count: patch_mask_count_kernel, one thread per patch of a strided grid, counts the nonzero bytes of a uint8 [T][H][W]
// mask under the patch (which patches overlap a hole, which avoid it).
//
// Weighted search (the patch nearest-neighbour generator's completeness normalisation, GPNN): score = float32(d2) * w_j with a
// per-reference-patch weight.  patchnn_min_kernel<true> is the same tile with another epilogue: |q_i|^2 is no longer constant
// along a row of scores, so the epilogue forms the whole d2 = |q_i|^2 + |r_j|^2 - 2 acc in int32 (the row norms of the tile
// wait in LDS), converts it (round to nearest even) and multiplies once in fp32.  A non-negative float's bit pattern orders
// like an unsigned integer, so the key (bits << 32) | j and the same atomic umin merge it; a row no comparison won (NaN
// weights, outside the contract) keeps its preset key and unpacks as score = +inf, nn = -1.
//
// Vote (the generator's fold): patch_vote_kernel rebuilds a volume from chosen patches as a gather, one thread per output voxel
// over the query-grid patches that cover it: no atomics, no zero fill, and integer sums, so the result is exact.
// patch_vote_wrap_kernel is the same gather over a periodic query grid (generate_patchnn --wrap).
//
// Tile: 128 x 128 per workgroup of four waves (each 64 x 64 = 2 x 2 MFMA tiles of 32 x 32), K step 64 bytes, both operands
// staged through LDS with 16-byte global loads (two LDS buffers: the next step's loads are in flight during the products, one
// barrier per step).  LDS rows are 80 bytes apart, so the 16 rows a quarter-wave reads lie on 16 different 16-byte bank slots.
// A and B fragments are read the same way from row-major [row][k] images (lane l: row l & 31, 16 bytes at k = 16 * (l >> 5)),
// so whatever order the instruction gives the 32 k values, both operands use the same one and the dot product is unaffected.
// That loop exists once, as pnn_tile_products: every search kernel here and in patchnn_prdc.inl is an epilogue around it, told
// who holds which row by pnn_lane / pnn_acc_row / pnn_row_norms.  Host: pnn_patch, pnn_pack_side, pnn_splits, pnn_ws.
//
// Exact sliced Wasserstein patch distance (the evaluate program's --swd): the same packed patch matrix against a small int8
// matrix of directions S[P][D] with entries in {-1, 0, +1}.  proj = sum_k S[p][k] * (byte[i][k] - 128) lies in
// [-128 D, +128 D], so bin = proj + 128 D indexes one of NB = 256 D + 1 bins and the whole metric is integer arithmetic.
//   4. patchproj_pack_dirs_kernel: S -> the GEMM's second operand [P padded to 128][D padded to 64, zeros], in the k order of
//      the patch pack (byte e of a row is byte e of the patch, (dt, dy, dx, c) raster), so the argument above keeps holding.
//   5. patchproj_zero_kernel: clears hist[P][NB] (the entry point never relies on the caller for that).
//   6. patchproj_hist_kernel: the NT GEMM of kernel 2 (pnn_tile_products on the direction tile) whose epilogue never stores
//      the N x P products: every accumulator element of a real patch (row < N: the tile padding's zero rows would land in
//      bin 128 D) and a real direction (p < P) increments hist[p][acc + 128 D] with a vector global atomic add.  Integer adds
//      are associative and commutative, so the histogram is independent of the launch geometry and of timing.
//   7. hist_w1_kernel: one workgroup per direction walks the NB bins of two histograms in chunks of 1024 with a carried block
//      prefix sum and accumulates num = sum_b |Nb cA(b) - Na cB(b)| = Na Nb W1 in 64 bits (exact while Na Nb 256 D < 2^63).
//
// Copied regions of a nearest-neighbour field (the evaluate program's --chunks): the connected components of the query patch
// grid under "6-neighbours whose nearest neighbours have the same displacement", by union-find in five launches on one stream
// (nnf_chunks_*_kernel below).  labels doubles as the parent array; every link points to a smaller index, so a tree's root is
// its smallest member and the labels are canonical without sorting.  The merge launch talks to other workgroups only through
// relaxed agent-scope atomics on parent (the XCDs' L2s are not coherent: a plain load may miss another XCD's atomicMin), it
// waits for nobody, and each of its loops strictly lowers an index per trip; whatever needs the finished forest is a later
// launch.  Sizes and statistics are integer atomic adds / max, so all outputs are independent of launch geometry and timing.
//
// Precision / recall / density / coverage of patch sets (the evaluate program's --prdc): patchnn_prdc.inl, included at the end,
// puts two more epilogues on kernel 2's tile: the k smallest distances of every patch within its own volume, and the number
// of keys whose per-key radius reaches a query.
//
// The pyramid's resize (generate_patchnn --antialias / --t-ratio, evaluate --scales): volresize.inl, included at the end, an exact
// antialiased resize of a uint8 volume in integer arithmetic, one gather kernel of its own.
//
// The feathered composite (generate / generate_patchnn --guide-mask): maskblend.inl, included at the end, a box dilation and a
// box count of a hole mask as 1-D passes, and the exact integer blend of two volumes under the resulting weights.
#include <limits.h>

#include <type_traits>

#include "hpvg_common.h"
#include "hpvg.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int PNN_TILE = 128;       // rows (query patches) and columns (reference patches) per workgroup tile
constexpr int PNN_BK = 64;          // bytes of K per step; patch rows are padded to a multiple of it
constexpr int PNN_LDS_ROW = 80;     // LDS row pitch in bytes (64 + 16)
constexpr int PNN_TARGET_WGS = 2048;  // the column range is split until the grid has about this many workgroups

struct PnnSide {
  int T, H, W;      // volume
  int nT, nY, nX;   // patch grid
  int st, sy, sx;   // stride
  long N;           // patches
  long Npad;        // padded to PNN_TILE
};

struct PnnPatch { int pt, ph, pw, D, Dp; };  // D bytes per patch, Dp padded to PNN_BK

struct PnnGeom {
  PnnSide q, r;
  PnnPatch p;
  long mq, mr;        // rows of the two packed matrices: the grids' patches, or the lengths of the subset search's lists
  long mqpad, mrpad;  // padded to PNN_TILE
  size_t off_qmat, off_rmat, off_qn, off_rn, off_keys, bytes;
};

inline bool pnn_side(PnnSide& s, int T, int H, int W, const int* patch, const int* stride) {
  if (T < 1 || H < 1 || W < 1 || !stride || stride[0] < 1 || stride[1] < 1 || stride[2] < 1) return false;
  if (patch[0] > T || patch[1] > H || patch[2] > W) return false;
  s.T = T; s.H = H; s.W = W;
  s.st = stride[0]; s.sy = stride[1]; s.sx = stride[2];
  s.nT = (T - patch[0]) / s.st + 1;
  s.nY = (H - patch[1]) / s.sy + 1;
  s.nX = (W - patch[2]) / s.sx + 1;
  const double n = (double)s.nT * (double)s.nY * (double)s.nX;
  if (n >= 2147483648.0) return false;
  s.N = (long)s.nT * s.nY * s.nX;
  s.Npad = (s.N + PNN_TILE - 1) / PNN_TILE * PNN_TILE;
  return true;
}

inline size_t pnn_align(size_t v) { return (v + 255) & ~(size_t)255; }

inline bool pnn_patch_ok(const int* patch) {
  if (!patch || patch[0] < 1 || patch[1] < 1 || patch[2] < 1) return false;
  const double d = 3.0 * (double)patch[0] * (double)patch[1] * (double)patch[2];
  return d * 65025.0 < 2147483648.0;
}

inline bool pnn_patch(PnnPatch& p, const int* patch) {
  if (!pnn_patch_ok(patch)) return false;
  p.pt = patch[0]; p.ph = patch[1]; p.pw = patch[2];
  p.D = 3 * p.pt * p.ph * p.pw;
  p.Dp = (p.D + PNN_BK - 1) / PNN_BK * PNN_BK;
  return true;
}

// the workspace of a search over mq query rows and mr reference rows
inline void pnn_layout(PnnGeom& g, long mq, long mr) {
  g.mq = mq; g.mr = mr;
  g.mqpad = (mq + PNN_TILE - 1) / PNN_TILE * PNN_TILE;
  g.mrpad = (mr + PNN_TILE - 1) / PNN_TILE * PNN_TILE;
  size_t o = 0;
  g.off_qmat = o; o = pnn_align(o + (size_t)g.mqpad * g.p.Dp);
  g.off_rmat = o; o = pnn_align(o + (size_t)g.mrpad * g.p.Dp);
  g.off_qn = o; o = pnn_align(o + (size_t)g.mqpad * 4);
  g.off_rn = o; o = pnn_align(o + (size_t)g.mrpad * 4);
  g.off_keys = o; o = pnn_align(o + (size_t)g.mqpad * 8);
  g.bytes = o;
}

// a list's length for the layout: the grid's count for a null list (given == false), 0 for a length the call refuses
inline long pnn_sel_rows(bool given, long n, long N) { return !given ? N : (n < 1 || n > N ? 0 : n); }

inline bool pnn_geom(PnnGeom& g, int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride,
                     const int* rstride) {
  if (!pnn_patch(g.p, patch)) return false;
  if (!pnn_side(g.q, Tq, Hq, Wq, patch, qstride) || !pnn_side(g.r, Tr, Hr, Wr, patch, rstride)) return false;
  pnn_layout(g, g.q.N, g.r.N);
  return true;
}

// one volume against P directions: the packed patches, then the packed directions
struct PpjGeom {
  PnnSide s;
  PnnPatch p;
  long Ppad;  // P padded to PNN_TILE
  long NB;    // 256 D + 1 bins
  size_t off_mat, off_dirs, bytes;
};

inline bool ppj_geom(PpjGeom& g, int T, int H, int W, const int* patch, const int* stride, int P) {
  if (!pnn_patch(g.p, patch) || P < 1 || !pnn_side(g.s, T, H, W, patch, stride)) return false;
  g.Ppad = ((long)P + PNN_TILE - 1) / PNN_TILE * PNN_TILE;
  g.NB = 256L * g.p.D + 1;
  size_t o = 0;
  g.off_mat = o; o = pnn_align(o + (size_t)g.s.Npad * g.p.Dp);
  g.off_dirs = o; o = pnn_align(o + (size_t)g.Ppad * g.p.Dp);
  g.bytes = o;
  return true;
}

// One wave per patch row: lane l writes the 4-byte words l, l + 64, ... of the row (zeros past D) and the wave sums the
// squares.  Rows past `rows` (tile padding) are all zeros.  sel == nullptr: row i is patch i of the grid (rows = s.N).  Otherwise
// row i is patch sel[i] (the gather of the subset search; rows = the list's length), clamped into [0, s.N).
__global__ __launch_bounds__(256) void patchnn_pack_kernel(const unsigned char* __restrict__ vol, signed char* __restrict__ mat,
                                                            int* __restrict__ norms, unsigned long long* __restrict__ keys,
                                                            PnnSide s, const int* __restrict__ sel, long rows, long rows_pad, int ph,
                                                            int pw, int D, int Dp) {
  const int lane = threadIdx.x & 63;
  const int run = pw * 3;  // contiguous bytes of one patch line
  const long wave0 = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  for (long row = wave0; row < rows_pad; row += (long)gridDim.x * 4) {
    unsigned* out = (unsigned*)(mat + row * Dp);
    int sq = 0;
    if (row < rows) {
      long p = row;
      if (sel) {
        p = sel[row];
        p = p < 0 ? 0 : (p >= s.N ? s.N - 1 : p);
      }
      const int gx = (int)(p % s.nX);
      const int gy = (int)((p / s.nX) % s.nY);
      const int gt = (int)(p / ((long)s.nX * s.nY));
      const unsigned char* base = vol + (((long)gt * s.st * s.H + (long)gy * s.sy) * s.W + (long)gx * s.sx) * 3;
      for (int w = lane; w < Dp / 4; w += 64) {
        unsigned word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int e = w * 4 + b;
          if (e < D) {
            const int line = e / run, off = e - line * run;
            const int dt = line / ph, dy = line - dt * ph;
            const int v = (int)base[((long)dt * s.H + dy) * s.W * 3 + off] - 128;
            sq += v * v;
            word |= (unsigned)(v & 0xff) << (8 * b);
          }
        }
        out[w] = word;
      }
    } else {
      for (int w = lane; w < Dp / 4; w += 64) out[w] = 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if (lane == 0) {
      if (norms) norms[row] = sq;
      if (keys) keys[row] = ~0ull;
    }
  }
}

__device__ __forceinline__ void pnn_load_tile(const signed char* __restrict__ A, const signed char* __restrict__ B, long arow0,
                                              long brow0, int Dp, int k0, int tid, i32x4 (&ra)[2], i32x4 (&rb)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = tid + 256 * u, row = c >> 2, kc = c & 3;
    ra[u] = *(const i32x4*)(A + (arow0 + row) * Dp + k0 + kc * 16);
    rb[u] = *(const i32x4*)(B + (brow0 + row) * Dp + k0 + kc * 16);
  }
}

__device__ __forceinline__ void pnn_store_tile(signed char* sa, signed char* sb, int tid, const i32x4 (&ra)[2],
                                               const i32x4 (&rb)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = tid + 256 * u, row = c >> 2, kc = c & 3;
    *(i32x4*)(sa + row * PNN_LDS_ROW + kc * 16) = ra[u];
    *(i32x4*)(sb + row * PNN_LDS_ROW + kc * 16) = rb[u];
  }
}

// Where a thread sits in the tile: wave (wr, wc) owns rows wr * 64.. and columns wc * 64.. of the 128 x 128 products; lane
// (lr, lh) holds column lr of each 32-wide MFMA tile and the rows pnn_acc_row(m, g, lh) of its 32-high ones.
struct PnnLane { int wr, wc, lr, lh; };

__device__ __forceinline__ PnnLane pnn_lane() {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  return {wave >> 1, wave & 1, lane & 31, lane >> 5};
}

// the row, within the wave's 64, that accumulator register g of MFMA tile m holds in a lane of half lh
__device__ __forceinline__ int pnn_acc_row(int m, int g, int lh) { return m * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh; }

// this lane's 32 row norms out of the tile's 128 in LDS: qrow[m][g >> 2][g & 3] belongs to row pnn_acc_row(m, g, lh)
__device__ __forceinline__ void pnn_row_norms(const int* qn_tile, int wr, int lh, i32x4 (&qrow)[2][4]) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int b = 0; b < 4; ++b) qrow[m][b] = *(const i32x4*)(qn_tile + wr * 64 + m * 32 + 8 * b + 4 * lh);
}

// One 128 x 128 tile of products: acc[m][n] of this wave's 64 x 64 quarter, rows arow0.. of A against rows brow0.. of B.  Two
// LDS buffers, the next step's global loads in flight during the products, one barrier per step; the closing barrier also covers
// buffer 0's last reads before the next call's first store: a workgroup walks on to its next column tile without another one.
__device__ __forceinline__ void pnn_tile_products(const signed char* __restrict__ A, const signed char* __restrict__ B, long arow0,
                                                  long brow0, int Dp, signed char (&lds)[2][2][PNN_TILE * PNN_LDS_ROW],
                                                  i32x16 (&acc)[2][2]) {
  const int tid = threadIdx.x;
  const PnnLane t = pnn_lane();
  const int nk = Dp / PNN_BK;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[m][n][g] = 0;

  i32x4 ra[2], rb[2];
  pnn_load_tile(A, B, arow0, brow0, Dp, 0, tid, ra, rb);
  pnn_store_tile(lds[0][0], lds[0][1], tid, ra, rb);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) pnn_load_tile(A, B, arow0, brow0, Dp, (kt + 1) * PNN_BK, tid, ra, rb);
    const signed char* sa = lds[cur][0] + (t.wr * 64 + t.lr) * PNN_LDS_ROW + t.lh * 16;
    const signed char* sb = lds[cur][1] + (t.wc * 64 + t.lr) * PNN_LDS_ROW + t.lh * 16;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      i32x4 fa[2], fb[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) fa[m] = *(const i32x4*)(sa + m * 32 * PNN_LDS_ROW + ks * 32);
#pragma unroll
      for (int n = 0; n < 2; ++n) fb[n] = *(const i32x4*)(sb + n * 32 * PNN_LDS_ROW + ks * 32);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }
    if (kt + 1 < nk) pnn_store_tile(lds[cur ^ 1][0], lds[cur ^ 1][1], tid, ra, rb);
    __syncthreads();
  }
}

// grid: (row tiles, column splits).  Workgroup (x, y) owns query rows [128 x, 128 x + 128) and walks the column tiles
// [y * tiles_per_split, (y + 1) * tiles_per_split) of the reference side.  WEIGHTED: the running minimum is the fp32 score
// float(d2) * rw[j] instead of the int32 d2 - |q|^2 (rw: [Nr], not padded).  Its epilogue holds 64 more values in flight: left
// alone the compiler takes 292 registers for it, i.e. one wave per SIMD; asked for the two waves the unweighted kernel runs at
// (232 registers) it fits 214 without spilling.  amdgpu_waves_per_eu(0) is clang's spelling of "no request" (the attribute is
// dropped), so the unweighted instantiation keeps its code.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WEIGHTED ? 2 : 0))) void patchnn_min_kernel(
    const signed char* __restrict__ A, const signed char* __restrict__ B, const int* __restrict__ qn, const int* __restrict__ rn,
    const float* __restrict__ rw, unsigned long long* __restrict__ keys, long Nq, long Nr, int Dp, int ncol_tiles,
    int tiles_per_split) {
  __shared__ __attribute__((aligned(16))) signed char lds[2][2][PNN_TILE * PNN_LDS_ROW];
  const int tid = threadIdx.x;
  const auto [wr, wc, lr, lh] = pnn_lane();
  const long arow0 = (long)blockIdx.x * PNN_TILE;
  const int jt0 = blockIdx.y * tiles_per_split;
  const int jt1 = min(jt0 + tiles_per_split, ncol_tiles);

  typename std::conditional<WEIGHTED, float, int>::type best[2][16];
  int bj[2][16];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      if constexpr (WEIGHTED) best[m][g] = __builtin_inff();
      else best[m][g] = INT_MAX;
      bj[m][g] = INT_MAX;
    }
  const int* qns = nullptr;
  if constexpr (WEIGHTED) {
    // the tile's row norms (padded rows exist); the K loop's barriers come before the first read
    __shared__ __attribute__((aligned(16))) int qn_tile[PNN_TILE];
    if (tid < PNN_TILE) qn_tile[tid] = qn[arow0 + tid];
    qns = qn_tile;
  }

  for (int jt = jt0; jt < jt1; ++jt) {
    const long brow0 = (long)jt * PNN_TILE;
    i32x16 acc[2][2];
    pnn_tile_products(A, B, arow0, brow0, Dp, lds, acc);

    // epilogue: this lane's column of each 32-wide tile against its running minima.  Columns are visited in ascending
    // order (jt, then n), so a strict < keeps the smallest index among equals.  qn is added once, after the merge.
    if constexpr (!WEIGHTED) {
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const long j = brow0 + wc * 64 + n * 32 + lr;
        const bool ok = j < Nr;
        const int rnj = rn[j];  // padded rows exist (norm 0)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const int s = ok ? rnj - 2 * acc[m][n][g] : INT_MAX;
            if (s < best[m][g]) {
              best[m][g] = s;
              bj[m][g] = (int)j;
            }
          }
      }
    } else {
      // weighted: the score depends on the row's norm too, so the whole exact d2 is formed here, converted (v_cvt_f32_i32
      // rounds to nearest even) and multiplied once.  A padded column gets the weight +inf: its score is +inf, or NaN where
      // d2 == 0, and neither passes the strict <; nor does a NaN weight.  No per-element branch.
      i32x4 qrow[2][4];
      pnn_row_norms(qns, wr, lh, qrow);
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const long j = brow0 + wc * 64 + n * 32 + lr;
        const int rnj = rn[j];
        const float wj = j < Nr ? rw[j] : __builtin_inff();  // rw has Nr entries, no padding
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const int d2 = qrow[m][g >> 2][g & 3] + rnj - 2 * acc[m][n][g];
            const float s = __fmul_rn((float)d2, wj);
            if (s < best[m][g]) {
              best[m][g] = s;
              bj[m][g] = (int)j;
            }
          }
      }
    }
  }

  // merge the 32 lanes (columns) of each row, then one atomic per row and wave.  Weighted: scores are >= +0 (or +inf), so
  // their bit patterns compare like the floats; a lane that never won carries (+inf, INT_MAX) and loses to every lane that
  // did, and a row nobody won keeps its preset key.
  using Key = typename std::conditional<WEIGHTED, unsigned, int>::type;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      Key b;
      if constexpr (WEIGHTED) b = __float_as_uint(best[m][g]);
      else b = best[m][g];
      int j = bj[m][g];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        const Key ob = (Key)__shfl_xor((int)b, o, 64);
        const int oj = __shfl_xor(j, o, 64);
        if (ob < b || (ob == b && oj < j)) {
          b = ob;
          j = oj;
        }
      }
      const long row = arow0 + wr * 64 + pnn_acc_row(m, g, lh);
      if constexpr (WEIGHTED) {
        if (lr == 0 && row < Nq && j != INT_MAX) atomicMin(&keys[row], ((unsigned long long)b << 32) | (unsigned)j);
      } else if (lr == 0 && row < Nq && b != INT_MAX) {
        const unsigned d2 = (unsigned)qn[row] + (unsigned)b;
        atomicMin(&keys[row], ((unsigned long long)d2 << 32) | (unsigned)j);
      }
    }
}

__global__ __launch_bounds__(256) void patchnn_unpack_kernel(const unsigned long long* __restrict__ keys, int* __restrict__ d2,
                                                              int* __restrict__ nn, long N) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    const unsigned long long k = keys[i];
    d2[i] = (int)(unsigned)(k >> 32);
    nn[i] = (int)(unsigned)(k & 0xffffffffull);
  }
}

// key -> score, nn of the weighted search; a key nobody lowered (see patchnn_min_kernel) gives +inf and -1
__global__ __launch_bounds__(256) void patchnn_unpack_weighted_kernel(const unsigned long long* __restrict__ keys,
                                                                       float* __restrict__ score, int* __restrict__ nn, long N) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    const unsigned long long k = keys[i];
    const bool none = k == ~0ull;
    score[i] = none ? __builtin_inff() : __uint_as_float((unsigned)(k >> 32));
    nn[i] = none ? -1 : (int)(unsigned)(k & 0xffffffffull);
  }
}

// every entry of the subset search's full-grid outputs starts as "not selected"
__global__ __launch_bounds__(256) void patchnn_fill_kernel(int* __restrict__ d2, int* __restrict__ nn, long N) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    d2[i] = -1;
    nn[i] = -1;
  }
}

// key of compacted row i -> d2, nn at grid patch qsel[i] (i itself for a null list), the winner's compacted index translated to
// its grid index rsel[j].  Both lists are clamped as the pack clamped them, so no write leaves the outputs and nn names the
// patch that was compared.  A key nobody lowered (no such row while mr >= 1) gives -1, -1.
__global__ __launch_bounds__(256) void patchnn_unpack_subset_kernel(const unsigned long long* __restrict__ keys,
                                                                     const int* __restrict__ qsel, const int* __restrict__ rsel,
                                                                     int* __restrict__ d2, int* __restrict__ nn, long mq, long Nq, long mr,
                                                                     long Nr) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < mq; i += (long)gridDim.x * 256) {
    const unsigned long long k = keys[i];
    long o = i;
    if (qsel) {
      o = qsel[i];
      o = o < 0 ? 0 : (o >= Nq ? Nq - 1 : o);
    }
    long j = (long)(unsigned)(k & 0xffffffffull);
    const bool none = k == ~0ull || j >= mr;
    if (!none && rsel) {
      j = rsel[j];
      j = j < 0 ? 0 : (j >= Nr ? Nr - 1 : j);
    }
    d2[o] = none ? -1 : (int)(unsigned)(k >> 32);
    nn[o] = none ? -1 : (int)j;
  }
}

// One thread per patch of the strided grid: the nonzero bytes of mask [T][H][W] under it.  Neighbouring threads read
// neighbouring bytes, and every byte is read from the cache by the up to pt * ph * pw patches that cover it.
__global__ __launch_bounds__(256) void patch_mask_count_kernel(const unsigned char* __restrict__ mask, int* __restrict__ count, PnnSide s,
                                                                int pt, int ph, int pw) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < s.N; i += (long)gridDim.x * 256) {
    const int gx = (int)(i % s.nX);
    const int gy = (int)((i / s.nX) % s.nY);
    const int gt = (int)(i / ((long)s.nX * s.nY));
    const unsigned char* base = mask + ((long)gt * s.st * s.H + (long)gy * s.sy) * s.W + (long)gx * s.sx;
    int c = 0;
    for (int dt = 0; dt < pt; ++dt)
      for (int dy = 0; dy < ph; ++dy) {
        const unsigned char* line = base + ((long)dt * s.H + dy) * s.W;
        for (int dx = 0; dx < pw; ++dx) c += line[dx] != 0;
      }
    count[i] = c;
  }
}

// One thread per output voxel (3 channels).  Along each axis the query-grid patches that cover coordinate c are
// g in [ceil((c - p + 1) / s), floor(c / s)] clipped to the grid, at offset d = c - g s inside the patch.
__global__ __launch_bounds__(256) void patch_vote_kernel(const unsigned char* __restrict__ v, const int* __restrict__ nn,
                                                          const unsigned char* __restrict__ fallback, unsigned char* __restrict__ out,
                                                          PnnSide q, PnnSide r, int pt, int ph, int pw) {
  const long total = (long)q.T * q.H * q.W;
  for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
    const int x = (int)(o % q.W);
    const int y = (int)((o / q.W) % q.H);
    const int t = (int)(o / ((long)q.W * q.H));
    const int gt0 = t < pt ? 0 : (t - pt) / q.st + 1, gt1 = min(t / q.st, q.nT - 1);
    const int gy0 = y < ph ? 0 : (y - ph) / q.sy + 1, gy1 = min(y / q.sy, q.nY - 1);
    const int gx0 = x < pw ? 0 : (x - pw) / q.sx + 1, gx1 = min(x / q.sx, q.nX - 1);
    int s0 = 0, s1 = 0, s2 = 0, cnt = 0;
    for (int gt = gt0; gt <= gt1; ++gt)
      for (int gy = gy0; gy <= gy1; ++gy)
        for (int gx = gx0; gx <= gx1; ++gx) {
          const int j = nn[((long)gt * q.nY + gy) * q.nX + gx];
          if (j < 0 || j >= r.N) continue;
          const int rx = j % r.nX, ry = (j / r.nX) % r.nY, rt = j / (r.nX * r.nY);
          const int vt = rt * r.st + (t - gt * q.st), vy = ry * r.sy + (y - gy * q.sy), vx = rx * r.sx + (x - gx * q.sx);
          const unsigned char* b = v + (((long)vt * r.H + vy) * r.W + vx) * 3;
          s0 += b[0];
          s1 += b[1];
          s2 += b[2];
          ++cnt;
        }
    unsigned char* dst = out + o * 3;
    if (cnt) {
      dst[0] = (unsigned char)((2 * s0 + cnt) / (2 * cnt));
      dst[1] = (unsigned char)((2 * s1 + cnt) / (2 * cnt));
      dst[2] = (unsigned char)((2 * s2 + cnt) / (2 * cnt));
    } else {
      dst[0] = fallback[o * 3];
      dst[1] = fallback[o * 3 + 1];
      dst[2] = fallback[o * 3 + 2];
    }
  }
}

// The vote onto a ring (hpvg_patch_vote_wrap_u8): q is the UNPADDED output with the sides of its periodic grid in nT / nY / nX
// (the whole side on a ring axis) and stride 1; bit ax of wm: axis ax is a ring.  Along a ring axis of side S the patches that
// cover coordinate c are g = (c - d) mod S for every offset d = 0 .. p - 1 (S >= p, so they are p different patches); along
// another axis g = c - d for the d with 0 <= g < n, as in patch_vote_kernel.  One thread per output voxel, d ascending.
__global__ __launch_bounds__(256) void patch_vote_wrap_kernel(const unsigned char* __restrict__ v, const int* __restrict__ nn,
                                                               const unsigned char* __restrict__ fallback,
                                                               unsigned char* __restrict__ out, PnnSide q, PnnSide r, int pt, int ph,
                                                               int pw, int wm) {
  const long total = (long)q.T * q.H * q.W;
  for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
    const int x = (int)(o % q.W);
    const int y = (int)((o / q.W) % q.H);
    const int t = (int)(o / ((long)q.W * q.H));
    // offsets d in [d0, d1] along each axis; on a ring every offset has its patch
    const int dt0 = (wm & 1) ? 0 : max(0, t - (q.nT - 1)), dt1 = (wm & 1) ? pt - 1 : min(pt - 1, t);
    const int dy0 = (wm & 2) ? 0 : max(0, y - (q.nY - 1)), dy1 = (wm & 2) ? ph - 1 : min(ph - 1, y);
    const int dx0 = (wm & 4) ? 0 : max(0, x - (q.nX - 1)), dx1 = (wm & 4) ? pw - 1 : min(pw - 1, x);
    int s0 = 0, s1 = 0, s2 = 0, cnt = 0;
    for (int dt = dt0; dt <= dt1; ++dt) {
      int gt = t - dt;
      if (gt < 0) gt += q.T;
      for (int dy = dy0; dy <= dy1; ++dy) {
        int gy = y - dy;
        if (gy < 0) gy += q.H;
        for (int dx = dx0; dx <= dx1; ++dx) {
          int gx = x - dx;
          if (gx < 0) gx += q.W;
          const int j = nn[((long)gt * q.nY + gy) * q.nX + gx];
          if (j < 0 || j >= r.N) continue;
          const int rx = j % r.nX, ry = (j / r.nX) % r.nY, rt = j / (r.nX * r.nY);
          const unsigned char* b = v + (((long)(rt * r.st + dt) * r.H + ry * r.sy + dy) * r.W + rx * r.sx + dx) * 3;
          s0 += b[0];
          s1 += b[1];
          s2 += b[2];
          ++cnt;
        }
      }
    }
    unsigned char* dst = out + o * 3;
    if (cnt) {
      dst[0] = (unsigned char)((2 * s0 + cnt) / (2 * cnt));
      dst[1] = (unsigned char)((2 * s1 + cnt) / (2 * cnt));
      dst[2] = (unsigned char)((2 * s2 + cnt) / (2 * cnt));
    } else {
      dst[0] = fallback[o * 3];
      dst[1] = fallback[o * 3 + 1];
      dst[2] = fallback[o * 3 + 2];
    }
  }
}

// One thread per 4-byte word of the packed direction matrix; rows past P and bytes past D are zeros.
__global__ __launch_bounds__(256) void patchproj_pack_dirs_kernel(const signed char* __restrict__ dirs, signed char* __restrict__ mat,
                                                                   int P, long Ppad, int D, int Dp) {
  const long wpr = Dp / 4, total = Ppad * wpr;
  for (long w = (long)blockIdx.x * 256 + threadIdx.x; w < total; w += (long)gridDim.x * 256) {
    const long p = w / wpr;
    const int kw = (int)(w - p * wpr);
    unsigned word = 0;
    if (p < P) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int e = kw * 4 + b;
        if (e < D) word |= (unsigned)(dirs[p * D + e] & 0xff) << (8 * b);
      }
    }
    ((unsigned*)mat)[w] = word;
  }
}

// p is 4-byte aligned: scalar stores up to the first 16-byte boundary and after the last, 16-byte stores between.
__global__ __launch_bounds__(256) void patchproj_zero_kernel(int* __restrict__ p, size_t n) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
  size_t head = (4 - (((uintptr_t)p >> 2) & 3)) & 3;
  if (head > n) head = n;
  const size_t nv = (n - head) / 4, tail0 = head + nv * 4;
  i32x4* v = (i32x4*)(p + head);
  const i32x4 z = {0, 0, 0, 0};
  for (size_t i = gid; i < nv; i += step) v[i] = z;
  if (gid < head) p[gid] = 0;
  if (gid < n - tail0) p[tail0 + gid] = 0;
}

// grid: row tiles of the patch matrix.  Workgroup x owns patches [128 x, 128 x + 128) and walks every tile of 128 directions, so
// its patch tile comes from HBM once and from the cache after that.  The MFMA's row operand is the direction tile and its
// column operand the patch tile: an accumulator register then holds one direction for the 32 patches of a half-wave, and the
// 32 increments of one atomic instruction land in one histogram row, near that direction's mean (measured 5-8 % faster than
// the other way round, where the 64 lanes of an instruction spread over 32 histogram rows).
__global__ __launch_bounds__(256) void patchproj_hist_kernel(const signed char* __restrict__ X, const signed char* __restrict__ S,
                                                              int* __restrict__ hist, long N, int P, int Dp, long NB, int offset,
                                                              int ndir_tiles) {
  __shared__ __attribute__((aligned(16))) signed char lds[2][2][PNN_TILE * PNN_LDS_ROW];
  const auto [wr, wc, lr, lh] = pnn_lane();
  const long xrow0 = (long)blockIdx.x * PNN_TILE;

  for (int jt = 0; jt < ndir_tiles; ++jt) {
    const long prow0 = (long)jt * PNN_TILE;
    i32x16 acc[2][2];
    pnn_tile_products(S, X, prow0, xrow0, Dp, lds, acc);

    // epilogue: one increment per accumulator element of a real patch and a real direction.  The bin is in range for
    // directions in {-1, 0, +1}; the range test keeps any other input from writing outside the histogram.
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const long i = xrow0 + wc * 64 + n * 32 + lr;  // this lane's patch
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const long p = prow0 + wr * 64 + pnn_acc_row(m, g, lh);  // this register's direction
          const long bin = (long)acc[m][n][g] + offset;
          if (i < N && p < P && bin >= 0 && bin < NB) atomicAdd(hist + (size_t)p * NB + bin, 1);
        }
      }
  }
}

// One workgroup per direction.  Thread t of a chunk of 1024 bins owns bins 4 t .. 4 t + 3; the two counts of a bin travel as
// one 64-bit word (A's in the high half, B's in the low half: the running sums stay below 2^31, so nothing carries across).
__global__ __launch_bounds__(256) void hist_w1_kernel(const int* __restrict__ histA, const int* __restrict__ histB, long long Na,
                                                       long long Nb, long NB, long long* __restrict__ num) {
  __shared__ unsigned long long wtot[2][4];
  __shared__ unsigned long long red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* a = histA + (size_t)blockIdx.x * NB;
  const int* b = histB + (size_t)blockIdx.x * NB;
  unsigned long long carry = 0, sum = 0;
  int it = 0;
  for (long base = 0; base < NB; base += 1024, ++it) {
    const long i0 = base + tid * 4;
    unsigned long long v[4], t = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i0 + i < NB) t += ((unsigned long long)(unsigned)a[i0 + i] << 32) | (unsigned)b[i0 + i];
      v[i] = t;
    }
    unsigned long long inc = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_up(inc, o, 64);
      if (lane >= o) inc += y;
    }
    if (lane == 63) wtot[it & 1][wave] = inc;
    __syncthreads();  // the other buffer is rewritten only after every thread has passed the next barrier
    unsigned long long pre = carry + (inc - t), tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned long long x = wtot[it & 1][w];
      if (w < wave) pre += x;
      tot += x;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i0 + i < NB) {
        const unsigned long long c = pre + v[i];
        const long long d = Nb * (long long)(c >> 32) - Na * (long long)(c & 0xffffffffull);
        sum += (unsigned long long)(d < 0 ? -d : d);
      }
    carry += tot;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (tid == 0) num[blockIdx.x] = (long long)(red[0] + red[1] + red[2] + red[3]);
}

}  // namespace

extern "C" {

int hpvg_patchnn_counts(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride, const int* rstride,
                        int* out3) {
  PnnGeom g;
  if (!out3 || !pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, qstride, rstride)) return HPVG_ERR_ARG;
  out3[0] = (int)g.q.N;
  out3[1] = (int)g.r.N;
  out3[2] = g.p.D;
  return HPVG_OK;
}

size_t hpvg_patchnn_ws_bytes(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride,
                             const int* rstride) {
  PnnGeom g;
  if (!pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, qstride, rstride)) return 0;
  return g.bytes;
}

}  // extern "C"

namespace {

// the pieces of a PnnGeom's workspace (the ball count's ends before keys)
struct PnnWs { signed char *qmat, *rmat; int *qn, *rn; unsigned long long* keys; };

inline PnnWs pnn_ws(const PnnGeom& g, void* ws) {
  char* w = (char*)ws;
  return {(signed char*)(w + g.off_qmat), (signed char*)(w + g.off_rmat), (int*)(w + g.off_qn), (int*)(w + g.off_rn),
          (unsigned long long*)(w + g.off_keys)};
}

// pack one side: patchnn_pack_kernel over rows_pad rows, one wave per row, at most 16384 workgroups
inline void pnn_pack_side(const unsigned char* vol, signed char* mat, int* norms, unsigned long long* keys, const PnnSide& side,
                          const int* sel, long rows, long rows_pad, const PnnPatch& p, hipStream_t st) {
  const long blocks = rows_pad / 4 < 16384 ? rows_pad / 4 : 16384;
  hipLaunchKernelGGL(patchnn_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, vol, mat, norms, keys, side, sel, rows, rows_pad,
                     p.ph, p.pw, p.D, p.Dp);
}

// the column splits of a search over nrt row tiles and nct column tiles: split until the grid has about PNN_TARGET_WGS
// workgroups, then even the splits out (per column tiles each)
inline void pnn_splits(long nrt, long nct, long& splits, long& per) {
  splits = (PNN_TARGET_WGS + nrt - 1) / nrt;
  if (splits > nct) splits = nct;
  if (splits < 1) splits = 1;
  per = (nct + splits - 1) / splits;
  splits = (nct + per - 1) / per;
}

// The vote's gather reads v, nn (nq entries) and fallback while other threads write out: whether out overlaps any of them.
inline bool pnn_vote_overlaps(const unsigned char* out, const unsigned char* fallback, const unsigned char* v, const int* nn,
                              size_t qvoxels, size_t rvoxels, long nq) {
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + qvoxels * 3;
  const uintptr_t in0[3] = {(uintptr_t)fallback, (uintptr_t)v, (uintptr_t)nn};
  const size_t inb[3] = {qvoxels * 3, rvoxels * 3, (size_t)nq * 4};
  for (int k = 0; k < 3; ++k)
    if (o0 < in0[k] + inb[k] && in0[k] < o1) return true;
  return false;
}

// pack both sides, the min kernel, unpack.  rweight == nullptr: d2 / nn into out0 (int); otherwise score / nn, out0 (float).
// qsel / rsel (unweighted only): the subset search's lists, g laid out for their lengths; both null is the whole-grid search.
int pnn_launch(const PnnGeom& g, const unsigned char* q, const unsigned char* r, const int* qsel, const int* rsel, const float* rweight,
               void* out0, int* nn, void* ws, void* stream) {
  const PnnWs w = pnn_ws(g, ws);
  hipStream_t st = (hipStream_t)stream;
  pnn_pack_side(q, w.qmat, w.qn, w.keys, g.q, qsel, g.mq, g.mqpad, g.p, st);
  pnn_pack_side(r, w.rmat, w.rn, nullptr, g.r, rsel, g.mr, g.mrpad, g.p, st);
  const long nrt = g.mqpad / PNN_TILE, nct = g.mrpad / PNN_TILE;
  long splits, per;
  pnn_splits(nrt, nct, splits, per);
  long ub = (g.q.N + 255) / 256;
  if (ub > 4096) ub = 4096;
  if (!rweight) {
    hipLaunchKernelGGL(patchnn_min_kernel<false>, dim3((unsigned)nrt, (unsigned)splits), dim3(256), 0, st, w.qmat, w.rmat, w.qn, w.rn,
                       (const float*)nullptr, w.keys, g.mq, g.mr, g.p.Dp, (int)nct, (int)per);
    if (!qsel && !rsel) {
      hipLaunchKernelGGL(patchnn_unpack_kernel, dim3((unsigned)ub), dim3(256), 0, st, w.keys, (int*)out0, nn, g.q.N);
    } else {
      if (qsel) hipLaunchKernelGGL(patchnn_fill_kernel, dim3((unsigned)ub), dim3(256), 0, st, (int*)out0, nn, g.q.N);
      long sb = (g.mq + 255) / 256;
      if (sb > 4096) sb = 4096;
      hipLaunchKernelGGL(patchnn_unpack_subset_kernel, dim3((unsigned)sb), dim3(256), 0, st, w.keys, qsel, rsel, (int*)out0, nn, g.mq,
                         g.q.N, g.mr, g.r.N);
    }
  } else {
    hipLaunchKernelGGL(patchnn_min_kernel<true>, dim3((unsigned)nrt, (unsigned)splits), dim3(256), 0, st, w.qmat, w.rmat, w.qn, w.rn,
                       rweight, w.keys, g.q.N, g.r.N, g.p.Dp, (int)nct, (int)per);
    hipLaunchKernelGGL(patchnn_unpack_weighted_kernel, dim3((unsigned)ub), dim3(256), 0, st, w.keys, (float*)out0, nn, g.q.N);
  }
  return hpvg_launch_status();
}

}  // namespace

extern "C" {

int hpvg_patchnn_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr, const int* patch,
                    const int* qstride, const int* rstride, int* d2, int* nn, void* ws, size_t ws_bytes, void* stream) {
  PnnGeom g;
  if (!q || !r || !d2 || !nn || !pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, qstride, rstride)) return HPVG_ERR_ARG;
  if (!ws || ws_bytes < g.bytes || ((uintptr_t)ws & 15)) return HPVG_ERR_WORKSPACE;
  return pnn_launch(g, q, r, nullptr, nullptr, nullptr, d2, nn, ws, stream);
}

int hpvg_patchnn_weighted_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr,
                             const int* patch, const int* qstride, const int* rstride, const float* rweight, float* score, int* nn,
                             void* ws, size_t ws_bytes, void* stream) {
  PnnGeom g;
  if (!q || !r || !rweight || !score || !nn || !pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, qstride, rstride)) return HPVG_ERR_ARG;
  if (!ws || ws_bytes < g.bytes || ((uintptr_t)ws & 15)) return HPVG_ERR_WORKSPACE;
  return pnn_launch(g, q, r, nullptr, nullptr, rweight, score, nn, ws, stream);
}

size_t hpvg_patchnn_subset_ws_bytes(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride,
                                    const int* rstride, long nqsel, long nrsel) {
  PnnGeom g;
  if (!pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, qstride, rstride)) return 0;
  const long mq = pnn_sel_rows(nqsel >= 0, nqsel, g.q.N), mr = pnn_sel_rows(nrsel >= 0, nrsel, g.r.N);
  if (!mq || !mr) return 0;
  pnn_layout(g, mq, mr);
  return g.bytes;
}

int hpvg_patchnn_subset_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr,
                           const int* patch, const int* qstride, const int* rstride, const int* qsel, long nqsel, const int* rsel,
                           long nrsel, int* d2, int* nn, void* ws, size_t ws_bytes, void* stream) {
  PnnGeom g;
  if (!q || !r || !d2 || !nn || !pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, qstride, rstride)) return HPVG_ERR_ARG;
  const long mq = pnn_sel_rows(qsel != nullptr, nqsel, g.q.N), mr = pnn_sel_rows(rsel != nullptr, nrsel, g.r.N);
  if (!mq || !mr) return HPVG_ERR_ARG;
  pnn_layout(g, mq, mr);
  if (!ws || ws_bytes < g.bytes || ((uintptr_t)ws & 15)) return HPVG_ERR_WORKSPACE;
  return pnn_launch(g, q, r, qsel, rsel, nullptr, d2, nn, ws, stream);
}

int hpvg_patch_mask_count_u8(const unsigned char* mask, int T, int H, int W, const int* patch, const int* stride, int* count,
                             void* stream) {
  PnnSide s;
  if (!mask || !count || !pnn_patch_ok(patch) || !pnn_side(s, T, H, W, patch, stride)) return HPVG_ERR_ARG;
  long blocks = (s.N + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(patch_mask_count_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mask, count, s, patch[0],
                     patch[1], patch[2]);
  return hpvg_launch_status();
}

int hpvg_patch_vote_counts(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride, const int* rstride,
                           long* out3) {
  PnnGeom g;
  if (!out3 || !pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, qstride, rstride)) return HPVG_ERR_ARG;
  // along one axis a grid of n patches of p at stride s covers (n - 1) s + p coordinates when s <= p, and n p otherwise
  const long ct = g.q.st <= g.p.pt ? (long)(g.q.nT - 1) * g.q.st + g.p.pt : (long)g.q.nT * g.p.pt;
  const long cy = g.q.sy <= g.p.ph ? (long)(g.q.nY - 1) * g.q.sy + g.p.ph : (long)g.q.nY * g.p.ph;
  const long cx = g.q.sx <= g.p.pw ? (long)(g.q.nX - 1) * g.q.sx + g.p.pw : (long)g.q.nX * g.p.pw;
  out3[0] = g.q.N;
  out3[1] = g.r.N;
  out3[2] = (long)Tq * Hq * Wq - ct * cy * cx;
  return HPVG_OK;
}

int hpvg_patch_vote_u8(const unsigned char* v, int Tr, int Hr, int Wr, const int* nn, int Tq, int Hq, int Wq, const int* patch,
                       const int* qstride, const int* rstride, const unsigned char* fallback, unsigned char* out, void* stream) {
  PnnGeom g;
  if (!v || !nn || !fallback || !out || !pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, qstride, rstride)) return HPVG_ERR_ARG;
  if (pnn_vote_overlaps(out, fallback, v, nn, (size_t)Tq * Hq * Wq, (size_t)Tr * Hr * Wr, g.q.N)) return HPVG_ERR_ARG;
  long blocks = ((long)Tq * Hq * Wq + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(patch_vote_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, v, nn, fallback, out, g.q, g.r,
                     g.p.pt, g.p.ph, g.p.pw);
  return hpvg_launch_status();
}

int hpvg_patch_vote_wrap_u8(const unsigned char* v, int Tr, int Hr, int Wr, const int* nn, int Tq, int Hq, int Wq, const int* patch,
                            const int* rstride, const int* wrap, const unsigned char* fallback, unsigned char* out, void* stream) {
  PnnGeom g;
  const int one[3] = {1, 1, 1};
  if (!v || !nn || !fallback || !out || !pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, one, rstride)) return HPVG_ERR_ARG;
  int wm = 0;
  for (int ax = 0; wrap && ax < 3; ++ax) {
    if (wrap[ax] != 0 && wrap[ax] != 1) return HPVG_ERR_ARG;
    wm |= wrap[ax] << ax;
  }
  // the periodic grid: the whole side on a ring axis (the geometry above has made sure that patch <= side)
  if (wm & 1) g.q.nT = Tq;
  if (wm & 2) g.q.nY = Hq;
  if (wm & 4) g.q.nX = Wq;
  if ((double)g.q.nT * (double)g.q.nY * (double)g.q.nX >= 2147483648.0) return HPVG_ERR_ARG;
  g.q.N = (long)g.q.nT * g.q.nY * g.q.nX;
  if (pnn_vote_overlaps(out, fallback, v, nn, (size_t)Tq * Hq * Wq, (size_t)Tr * Hr * Wr, g.q.N)) return HPVG_ERR_ARG;
  long blocks = ((long)Tq * Hq * Wq + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(patch_vote_wrap_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, v, nn, fallback, out, g.q, g.r,
                     g.p.pt, g.p.ph, g.p.pw, wm);
  return hpvg_launch_status();
}

size_t hpvg_patchproj_bins(const int* patch) {
  if (!pnn_patch_ok(patch)) return 0;
  return (size_t)256 * 3 * patch[0] * patch[1] * patch[2] + 1;
}

size_t hpvg_patchproj_ws_bytes(int T, int H, int W, const int* patch, const int* stride, int P) {
  PpjGeom g;
  if (!ppj_geom(g, T, H, W, patch, stride, P)) return 0;
  return g.bytes;
}

int hpvg_patchproj_hist_u8(const unsigned char* vol, int T, int H, int W, const int* patch, const int* stride, const signed char* dirs,
                           int P, int* hist, void* ws, size_t ws_bytes, void* stream) {
  PpjGeom g;
  if (!vol || !dirs || !hist || ((uintptr_t)hist & 3) || !ppj_geom(g, T, H, W, patch, stride, P)) return HPVG_ERR_ARG;
  if (!ws || ws_bytes < g.bytes || ((uintptr_t)ws & 15)) return HPVG_ERR_WORKSPACE;
  signed char* mat = (signed char*)ws + g.off_mat;
  signed char* dmat = (signed char*)ws + g.off_dirs;
  hipStream_t st = (hipStream_t)stream;
  pnn_pack_side(vol, mat, nullptr, nullptr, g.s, nullptr, g.s.N, g.s.Npad, g.p, st);
  long dblocks = (g.Ppad * (g.p.Dp / 4) + 255) / 256;
  if (dblocks > 4096) dblocks = 4096;
  hipLaunchKernelGGL(patchproj_pack_dirs_kernel, dim3((unsigned)dblocks), dim3(256), 0, st, dirs, dmat, P, g.Ppad, g.p.D, g.p.Dp);
  const size_t nh = (size_t)P * g.NB;
  size_t zblocks = (nh / 4 + 255) / 256 + 1;
  if (zblocks > 8192) zblocks = 8192;
  hipLaunchKernelGGL(patchproj_zero_kernel, dim3((unsigned)zblocks), dim3(256), 0, st, hist, nh);
  hipLaunchKernelGGL(patchproj_hist_kernel, dim3((unsigned)(g.s.Npad / PNN_TILE)), dim3(256), 0, st, mat, dmat, hist, g.s.N, P, g.p.Dp,
                     g.NB, 128 * g.p.D, (int)(g.Ppad / PNN_TILE));
  return hpvg_launch_status();
}

int hpvg_hist_w1_i32(const int* histA, long Na, const int* histB, long Nb, int P, long NB, long long* num, void* stream) {
  if (!histA || !histB || !num || P < 1 || Na < 1 || Nb < 1 || Na >= 2147483648L || Nb >= 2147483648L) return HPVG_ERR_ARG;
  if (NB < 769 || (NB - 1) % 768 != 0 || (double)(NB - 1) / 256.0 * 65025.0 >= 2147483648.0) return HPVG_ERR_ARG;  // 256 D + 1, D = 3 pt ph pw
  if ((unsigned __int128)Na * (unsigned __int128)Nb * (unsigned __int128)(NB - 1) >= ((unsigned __int128)1 << 63)) return HPVG_ERR_ARG;
  hipLaunchKernelGGL(hist_w1_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, histA, histB, (long long)Na, (long long)Nb,
                     NB, num);
  return hpvg_launch_status();
}

}  // extern "C"

namespace {

struct NnfGeom {
  int gT, gH, gW;  // query patch grid
  int kT, kH, kW;  // key patch grid
  int qst, qsy, qsx;
  int rst, rsy, rsx;
  long Nq, Nr;
};

constexpr int NNF_MAX_BLOCKS = 8192;  // grid-stride past this many workgroups of 256

// Whether patch i = (t, y, x) of the query grid is kept, and its displacement in voxels (b * rstride - a * qstride per axis, in
// 64 bits: a product of two ints cannot overflow).  nn[i] is only decoded, never used as an address.
__device__ __forceinline__ bool nnf_disp(const int* __restrict__ nn, const int* __restrict__ d2, int max_d2, const NnfGeom& g, long i,
                                         int t, int y, int x, long long& dt, long long& dy, long long& dx) {
  const int j = nn[i];
  if (j < 0 || j >= g.Nr) return false;
  if (d2) {
    const int d = d2[i];
    if (d < 0 || d > max_d2) return false;
  }
  const unsigned kw = (unsigned)g.kW, khw = (unsigned)g.kH * (unsigned)g.kW;  // kH kW <= Nr < 2^31
  const unsigned bt = (unsigned)j / khw, rem = (unsigned)j - bt * khw;
  const unsigned by = rem / kw, bx = rem - by * kw;
  dt = (long long)bt * g.rst - (long long)t * g.qst;
  dy = (long long)by * g.rsy - (long long)y * g.qsy;
  dx = (long long)bx * g.rsx - (long long)x * g.qsx;
  return true;
}

__device__ __forceinline__ void nnf_coords(const NnfGeom& g, long i, int& t, int& y, int& x) {
  const unsigned gw = (unsigned)g.gW, ghw = (unsigned)g.gH * (unsigned)g.gW;  // gH gW <= Nq < 2^31
  const unsigned ut = (unsigned)i / ghw, rem = (unsigned)i - ut * ghw;
  const unsigned uy = rem / gw;
  t = (int)ut;
  y = (int)uy;
  x = (int)(rem - uy * gw);
}

__device__ __forceinline__ unsigned long long nnf_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// launch 1: parent[i] = i for a kept patch and -1 otherwise; sizes and stats are cleared here (no memset node)
__global__ __launch_bounds__(256) void nnf_chunks_init_kernel(const int* __restrict__ nn, const int* __restrict__ d2, int max_d2,
                                                               NnfGeom g, int* __restrict__ parent, int* __restrict__ sizes,
                                                               long long* __restrict__ stats) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid < 6) stats[gid] = 0;
  for (long i = gid; i < g.Nq; i += (long)gridDim.x * 256) {
    const int j = nn[i];
    bool kept = j >= 0 && j < g.Nr;
    if (kept && d2) {
      const int d = d2[i];
      kept = d >= 0 && d <= max_d2;
    }
    parent[i] = kept ? (int)i : -1;
    sizes[i] = 0;
  }
}

// The root of x's tree as far as this thread can see it.  Every value ever stored in parent[x] of a kept patch is in [0, x]
// (launch 1 stores x, the merge only lowers it with atomicMin), so every trip of the loop strictly lowers x: it ends after at
// most x trips whatever other workgroups do.  The load is a relaxed agent-scope atomic, so it is served past this CU's L1 and
// sees atomics from the other XCDs; a value that is stale all the same is an earlier parent, i.e. still a member of the tree.
__device__ __forceinline__ int nnf_find(int* parent, int x) {
  for (;;) {
    const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= x || p < 0) return x;  // p == x: a root (the other two cannot happen; they only keep a misused buffer in bounds)
    x = p;
  }
}

// Join the trees of a and b: the larger root is linked under the smaller one with atomicMin.  A trip that does not return
// has found parent[a] already lowered by somebody else (old < a) and carries on with (old, b): the atomicMin left a under
// min(old, b), so joining old and b is exactly what is still owed.  Each such trip replaces the larger of the two indices by a
// strictly smaller one (the finds only lower them too), so a + b strictly decreases and the loop ends whatever other
// workgroups do; nothing here waits for another thread.
__device__ __forceinline__ void nnf_unite(int* parent, int a, int b) {
  for (;;) {
    a = nnf_find(parent, a);
    b = nnf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;  // a was still a root and now hangs under b
    a = old;
  }
}

// launch 2: one thread per patch and its three forward pairs; kept, in_place and coherent_pairs are counted on the way and leave
// as one 64-bit atomic per block and counter.  No path compression: parent is touched only by the loads and atomicMins above.
__global__ __launch_bounds__(256) void nnf_chunks_merge_kernel(const int* __restrict__ nn, const int* __restrict__ d2, int max_d2,
                                                                NnfGeom g, int* parent, long long* __restrict__ stats) {
  __shared__ unsigned long long red[3][4];
  unsigned long long kept = 0, inplace = 0, coh = 0;
  const long plane = (long)g.gH * g.gW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < g.Nq; i += (long)gridDim.x * 256) {
    int t, y, x;
    nnf_coords(g, i, t, y, x);
    long long dt, dy, dx, et, ey, ex;
    if (!nnf_disp(nn, d2, max_d2, g, i, t, y, x, dt, dy, dx)) continue;
    ++kept;
    inplace += (dt | dy | dx) == 0;
    if (x + 1 < g.gW && nnf_disp(nn, d2, max_d2, g, i + 1, t, y, x + 1, et, ey, ex) && et == dt && ey == dy && ex == dx) {
      ++coh;
      nnf_unite(parent, (int)i, (int)(i + 1));
    }
    if (y + 1 < g.gH && nnf_disp(nn, d2, max_d2, g, i + g.gW, t, y + 1, x, et, ey, ex) && et == dt && ey == dy && ex == dx) {
      ++coh;
      nnf_unite(parent, (int)i, (int)(i + g.gW));
    }
    if (t + 1 < g.gT && nnf_disp(nn, d2, max_d2, g, i + plane, t + 1, y, x, et, ey, ex) && et == dt && ey == dy && ex == dx) {
      ++coh;
      nnf_unite(parent, (int)i, (int)(i + plane));
    }
  }
  kept = nnf_wave_sum(kept);
  inplace = nnf_wave_sum(inplace);
  coh = nnf_wave_sum(coh);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = kept;
    red[1][wave] = inplace;
    red[2][wave] = coh;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const unsigned long long v = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    if (v) atomicAdd((unsigned long long*)stats + threadIdx.x, v);
  }
}

// launch 3: label = root, in place.  The forest is final (launch 2 is over), so a racing reader finds in labels[k] either k's
// parent or k's root, both on the way to the same root; the loop of nnf_find ends for the reason given there.
__global__ __launch_bounds__(256) void nnf_chunks_flatten_kernel(int* labels, long N) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    const int p = __hip_atomic_load(labels + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p < 0 || p == (int)i) continue;
    const int r = nnf_find(labels, p);
    if (r != p) __hip_atomic_store(labels + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// launch 4: sizes[label] += 1.  The lanes of a wave that share a label leave as one add: a rigid copy is ONE chunk, and one
// atomic per patch on one word would serialise the whole grid.  The inner loop clears at least its leader's bit per trip and
// involves this wave only.
__global__ __launch_bounds__(256) void nnf_chunks_size_kernel(const int* __restrict__ labels, int* __restrict__ sizes, long N) {
  const int lane = threadIdx.x & 63;
  for (long base = (long)blockIdx.x * 256; base < N; base += (long)gridDim.x * 256) {  // uniform trip count per wave
    const long i = base + threadIdx.x;
    const int l = i < N ? labels[i] : -1;
    unsigned long long todo = __ballot(l >= 0 && l < N);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int ll = __shfl(l, leader, 64);
      const unsigned long long same = __ballot(l == ll) & todo;
      if (lane == leader) atomicAdd(sizes + ll, __popcll(same));
      todo &= ~same;
    }
  }
}

// launch 5: chunks, largest, sum_sq over the roots (labels[i] == i), reduced per block before one 64-bit atomic each
__global__ __launch_bounds__(256) void nnf_chunks_stats_kernel(const int* __restrict__ labels, const int* __restrict__ sizes, long N,
                                                                long long* __restrict__ stats) {
  __shared__ unsigned long long red[3][4];
  unsigned long long chunks = 0, largest = 0, sumsq = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    if (labels[i] != (int)i) continue;
    const unsigned long long s = (unsigned long long)(unsigned)sizes[i];
    ++chunks;
    largest = s > largest ? s : largest;
    sumsq += s * s;
  }
  chunks = nnf_wave_sum(chunks);
  sumsq = nnf_wave_sum(sumsq);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long v = __shfl_xor(largest, o, 64);
    largest = v > largest ? v : largest;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = chunks;
    red[1][wave] = largest;
    red[2][wave] = sumsq;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long c = 0, m = 0, q = 0;
    for (int w = 0; w < 4; ++w) {
      c += red[0][w];
      m = red[1][w] > m ? red[1][w] : m;
      q += red[2][w];
    }
    if (c) {
      atomicAdd((unsigned long long*)stats + 3, c);
      atomicMax((unsigned long long*)stats + 4, m);
      atomicAdd((unsigned long long*)stats + 5, q);
    }
  }
}

}  // namespace

extern "C" {

int hpvg_nnf_chunks_i32(const int* nn, const int* d2, int max_d2, const int* qgrid, const int* rgrid, const int* qstride,
                        const int* rstride, int* labels, int* sizes, long long* stats, void* stream) {
  if (!nn || !labels || !sizes || !stats || !qgrid || !rgrid || !qstride || !rstride) return HPVG_ERR_ARG;
  for (int a = 0; a < 3; ++a)
    if (qgrid[a] < 1 || rgrid[a] < 1 || qstride[a] < 1 || rstride[a] < 1) return HPVG_ERR_ARG;
  if ((double)qgrid[0] * (double)qgrid[1] * (double)qgrid[2] >= 2147483648.0) return HPVG_ERR_ARG;
  if ((double)rgrid[0] * (double)rgrid[1] * (double)rgrid[2] >= 2147483648.0) return HPVG_ERR_ARG;
  if (d2 && max_d2 < 0) return HPVG_ERR_ARG;
  NnfGeom g;
  g.gT = qgrid[0]; g.gH = qgrid[1]; g.gW = qgrid[2];
  g.kT = rgrid[0]; g.kH = rgrid[1]; g.kW = rgrid[2];
  g.qst = qstride[0]; g.qsy = qstride[1]; g.qsx = qstride[2];
  g.rst = rstride[0]; g.rsy = rstride[1]; g.rsx = rstride[2];
  g.Nq = (long)g.gT * g.gH * g.gW;
  g.Nr = (long)g.kT * g.kH * g.kW;
  long blocks = (g.Nq + 255) / 256;
  if (blocks > NNF_MAX_BLOCKS) blocks = NNF_MAX_BLOCKS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nnf_chunks_init_kernel, dim3((unsigned)blocks), dim3(256), 0, st, nn, d2, max_d2, g, labels, sizes, stats);
  hipLaunchKernelGGL(nnf_chunks_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, st, nn, d2, max_d2, g, labels, stats);
  hipLaunchKernelGGL(nnf_chunks_flatten_kernel, dim3((unsigned)blocks), dim3(256), 0, st, labels, g.Nq);
  hipLaunchKernelGGL(nnf_chunks_size_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const int*)labels, sizes, g.Nq);
  hipLaunchKernelGGL(nnf_chunks_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const int*)labels, (const int*)sizes, g.Nq,
                     stats);
  return hpvg_launch_status();
}

}  // extern "C"

// evaluate --prdc: the self k-nearest search and the ball count, two more epilogues on the tile above
#include "patchnn_prdc.inl"

// generate_patchnn --search patchmatch: the deterministic approximate search (its own kernel; shares the geometry above)
#include "patchmatch.inl"

// generate_patchnn --antialias / --t-ratio, evaluate --scales: the exact antialiased volume resize (its own gather kernel)
#include "volresize.inl"

// generate --guide-mask, generate_patchnn --guide-mask: the dilate-and-feather composite of two byte volumes (1-D passes)
#include "maskblend.inl"
