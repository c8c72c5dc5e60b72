// Included at the end of patchnn.hip: the two searches behind evaluate --prdc (improved precision / recall, Kynkaanniemi et al.
// 2019; density / coverage, Naeem et al. 2020, on raw patches).  Both are further epilogues on patchnn_min_kernel's tile: the
// pack kernel (pnn_pack_side), the 128 x 128 tile of four waves with its LDS images, K loop and double buffering
// (pnn_tile_products), the lane coordinates (pnn_lane, pnn_acc_row, pnn_row_norms) and the column splits (pnn_splits) are
// those of patchnn.hip; only what happens to the 64 x 64 accumulators of a wave differs.
//
// Self k-nearest (patchknn_self_kernel<KC>): one volume, A = B = its packed patch matrix.  For every row i the k smallest
// d2(i, j) over j != i, j < N, ascending and with multiplicity (the exclusion is by index: another patch at distance 0
// counts).  One GEMM pass; the N x N products are never stored.  Each lane keeps, for each of its 32 rows, a sorted list of
// KC values s = |r_j|^2 - 2 q_i.r_j (capacity KC = 4 or 8 >= k, padded with INT_MAX; |q_i|^2 is constant along a row and is
// added at the end).  A candidate enters through a chain of KC min / max pairs; a wave-uniform test (does any lane's
// candidate beat its row's worst kept value?) skips the chain, and after the first few column tiles it nearly always does.
// At the end the 32 lanes of a row merge their lists by an xor butterfly of shuffles, and the wave writes its rows' lists to
// part [2 * blockIdx.y + (wave & 1)] of the workspace, laid out [part][row][KC].  Every (part, row < N) is written by exactly
// one wave, nobody waits for anybody, and patchknn_merge_kernel (one thread per row) merges the parts, adds |q_i|^2 and writes
// the first k.  The k smallest elements of a union of integer multisets do not depend on how the union was split or in which
// order it was merged, so the result is independent of the launch geometry and of timing.
//
// Ball count (patchnn_ball_count_kernel): query matrix against key matrix with an int32 radius per key,
// count[i] = #{j < Nr : d2(q_i, r_j) <= rad[j]}.  As in patchnn_min_kernel<true> the row norms of the tile wait in LDS and the
// test uses the whole exact int32 distance: |q_i|^2 + |r_j|^2 - 2 acc <= rad[j], evaluated as |q_i|^2 - 2 acc <= rad[j] - |r_j|^2
// (rad >= 0 and the norms are bounded by D * 128^2, so neither side can overflow).  A padded column gets the threshold -1,
// below every left side (its products are 0 and |q_i|^2 >= 0), so it never counts and there is no per-element branch.  Each lane
// counts for its 32 rows over the column tiles its workgroup walks, the 32 lanes of a row add up by shuffles and the wave does
// one integer atomicAdd per row into count, which a launch of the entry point's own has cleared.  Integer adds are associative
// and commutative, so the result is independent of the launch geometry and of timing.

namespace {

// s into the ascending list: every slot keeps the smaller of itself and the travelling value, which leaves as the larger
template <int KC>
__device__ __forceinline__ void knn_insert(int (&list)[KC], int s) {
#pragma unroll
  for (int t = 0; t < KC; ++t) {
    const int lo = min(list[t], s);
    s = max(list[t], s);
    list[t] = lo;
  }
}

// This lane's ascending list and that of lane ^ o -> the KC smallest of both, ascending, in both lanes: min(mine[t],
// theirs[KC - 1 - t]) over t holds exactly those KC values as a bitonic sequence (the first half-cleaner of a bitonic merge of
// 2 KC values), and log2(KC) more half-cleaners sort it.  The two lanes form the same multiset, so they end up equal.
template <int KC>
__device__ __forceinline__ void knn_merge_lane(int (&list)[KC], int o) {
  int other[KC];
#pragma unroll
  for (int t = 0; t < KC; ++t) other[t] = __shfl_xor(list[t], o, 64);
#pragma unroll
  for (int t = 0; t < KC; ++t) list[t] = min(list[t], other[KC - 1 - t]);
#pragma unroll
  for (int h = KC / 2; h > 0; h >>= 1)
#pragma unroll
    for (int t = 0; t < KC; ++t)
      if ((t & h) == 0) {
        const int lo = min(list[t], list[t + h]), hi = max(list[t], list[t + h]);
        list[t] = lo;
        list[t + h] = hi;
      }
}

// grid: (row tiles, column splits), as patchnn_min_kernel.  parts: [2 * gridDim.y][Npad][KC].  A lane holds 32 * KC list values
// beside the 64 accumulators.  KC = 4: left alone the compiler takes 292 registers (one wave per SIMD, 219 ms at 379 500
// patches); asked for two waves it fits 256 without scratch and runs in 132 ms (profiles/prdc_perf.txt).  KC = 8 cannot: its
// 256 list values alone fill a two-wave budget, so it asks for the one wave per SIMD that 512 registers per lane are.
template <int KC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KC > 4 ? 1 : 2))) void patchknn_self_kernel(
    const signed char* __restrict__ X, const int* __restrict__ xn, int* __restrict__ parts, long N, long Npad, int Dp, int ncol_tiles,
    int tiles_per_split) {
  __shared__ __attribute__((aligned(16))) signed char lds[2][2][PNN_TILE * PNN_LDS_ROW];
  const auto [wr, wc, lr, lh] = pnn_lane();
  const long arow0 = (long)blockIdx.x * PNN_TILE;
  const int jt0 = blockIdx.y * tiles_per_split;
  const int jt1 = min(jt0 + tiles_per_split, ncol_tiles);

  int list[2][16][KC];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int g = 0; g < 16; ++g)
#pragma unroll
      for (int t = 0; t < KC; ++t) list[m][g][t] = INT_MAX;
  // register g of tile m is row rbase + pnn_acc_row(m, g, 0) of the matrix (the lane half folded into the base)
  const int rbase = (int)arow0 + wr * 64 + 4 * lh;

  for (int jt = jt0; jt < jt1; ++jt) {
    const long brow0 = (long)jt * PNN_TILE;
    i32x16 acc[2][2];
    pnn_tile_products(X, X, arow0, brow0, Dp, lds, acc);

    // epilogue: this lane's column of each 32-wide tile against its rows' lists.  A padded column and, on the diagonal tile,
    // the row's own column carry INT_MAX, which no list's worst value exceeds.
    const bool diag = jt == (int)blockIdx.x;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int j = (int)brow0 + wc * 64 + n * 32 + lr;
      const bool ok = j < N;
      const int rnj = xn[j];  // padded rows exist (norm 0)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int row = rbase + pnn_acc_row(m, g, 0);
          const int s = ok && !(diag && j == row) ? rnj - 2 * acc[m][n][g] : INT_MAX;
          if (__any(s < list[m][g][KC - 1])) knn_insert<KC>(list[m][g], s);
        }
    }
  }

  // merge the 32 lanes (columns) of each row: after the butterfly every lane of a half-wave holds the row's list
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) knn_merge_lane<KC>(list[m][g], o);
      const long row = (long)rbase + pnn_acc_row(m, g, 0);
      if (lr == 0 && row < N) {
        i32x4* dst = (i32x4*)(parts + (((size_t)(2 * blockIdx.y + wc)) * Npad + row) * KC);
#pragma unroll
        for (int t = 0; t < KC; t += 4) {
          const i32x4 v = {list[m][g][t], list[m][g][t + 1], list[m][g][t + 2], list[m][g][t + 3]};
          dst[t / 4] = v;
        }
      }
    }
}

// One thread per row: the k smallest of the row's nparts lists, plus |q_i|^2.  N > k, so the first k merged values are real.
template <int KC>
__global__ __launch_bounds__(256) void patchknn_merge_kernel(const int* __restrict__ parts, const int* __restrict__ xn,
                                                              int* __restrict__ kth, long N, long Npad, int nparts, int k) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    int list[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) list[t] = INT_MAX;
    for (int p = 0; p < nparts; ++p) {
      const i32x4* src = (const i32x4*)(parts + ((size_t)p * Npad + i) * KC);
#pragma unroll
      for (int t = 0; t < KC; t += 4) {
        const i32x4 v = src[t / 4];
#pragma unroll
        for (int e = 0; e < 4; ++e) knn_insert<KC>(list, v[e]);
      }
    }
    const int qn = xn[i];
#pragma unroll
    for (int t = 0; t < KC; ++t)
      if (t < k) kth[i * k + t] = qn + list[t];
  }
}

// grid: (row tiles, column splits), as patchnn_min_kernel.  rad: [Nr], not padded.  The counters add 32 values to the
// accumulators' 64, as the weighted search's epilogue does, and the same request for two waves per SIMD applies.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void patchnn_ball_count_kernel(
    const signed char* __restrict__ A, const signed char* __restrict__ B, const int* __restrict__ qn, const int* __restrict__ rn,
    const int* __restrict__ rad, int* __restrict__ count, long Nq, long Nr, int Dp, int ncol_tiles, int tiles_per_split) {
  __shared__ __attribute__((aligned(16))) signed char lds[2][2][PNN_TILE * PNN_LDS_ROW];
  __shared__ __attribute__((aligned(16))) int qn_tile[PNN_TILE];
  const int tid = threadIdx.x;
  const auto [wr, wc, lr, lh] = pnn_lane();
  const long arow0 = (long)blockIdx.x * PNN_TILE;
  const int jt0 = blockIdx.y * tiles_per_split;
  const int jt1 = min(jt0 + tiles_per_split, ncol_tiles);

  // the tile's row norms (padded rows exist); the K loop's barriers come before the first read
  if (tid < PNN_TILE) qn_tile[tid] = qn[arow0 + tid];
  int cnt[2][16];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int g = 0; g < 16; ++g) cnt[m][g] = 0;

  for (int jt = jt0; jt < jt1; ++jt) {
    const long brow0 = (long)jt * PNN_TILE;
    i32x16 acc[2][2];
    pnn_tile_products(A, B, arow0, brow0, Dp, lds, acc);

    i32x4 qrow[2][4];
    pnn_row_norms(qn_tile, wr, lh, qrow);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const long j = brow0 + wc * 64 + n * 32 + lr;
      const int thr = j < Nr ? rad[j] - rn[j] : -1;  // rad has Nr entries, no padding
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int g = 0; g < 16; ++g) cnt[m][g] += (qrow[m][g >> 2][g & 3] - 2 * acc[m][n][g] <= thr) ? 1 : 0;
    }
  }

  // add up the 32 lanes (columns) of each row, then one atomic per row and wave
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      int c = cnt[m][g];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
      const long row = arow0 + wr * 64 + pnn_acc_row(m, g, lh);
      if (lr == 0 && row < Nq && c != 0) atomicAdd(&count[row], c);
    }
}

// one volume against itself: the packed patches, their norms, then the partial lists [2 * splits][Npad][KC]
struct KnnGeom {
  PnnSide s;
  PnnPatch p;
  int KC;
  long splits, per;
  size_t off_mat, off_norms, off_parts, bytes;
};

inline bool knn_geom(KnnGeom& g, int T, int H, int W, const int* patch, const int* stride, int k) {
  if (k < 1 || k > 8 || !pnn_patch(g.p, patch) || !pnn_side(g.s, T, H, W, patch, stride) || g.s.N <= k) return false;
  g.KC = k <= 4 ? 4 : 8;
  const long nt = g.s.Npad / PNN_TILE;
  pnn_splits(nt, nt, g.splits, g.per);
  size_t o = 0;
  g.off_mat = o; o = pnn_align(o + (size_t)g.s.Npad * g.p.Dp);
  g.off_norms = o; o = pnn_align(o + (size_t)g.s.Npad * 4);
  g.off_parts = o; o = pnn_align(o + (size_t)(2 * g.splits) * g.s.Npad * g.KC * 4);
  g.bytes = o;
  return true;
}

template <int KC>
void knn_launch(const KnnGeom& g, const signed char* mat, const int* norms, int* parts, int* kth, int k, hipStream_t st) {
  const long nt = g.s.Npad / PNN_TILE;
  hipLaunchKernelGGL(patchknn_self_kernel<KC>, dim3((unsigned)nt, (unsigned)g.splits), dim3(256), 0, st, mat, norms, parts, g.s.N,
                     g.s.Npad, g.p.Dp, (int)nt, (int)g.per);
  long mb = (g.s.N + 255) / 256;
  if (mb > 4096) mb = 4096;
  hipLaunchKernelGGL(patchknn_merge_kernel<KC>, dim3((unsigned)mb), dim3(256), 0, st, (const int*)parts, norms, kth, g.s.N, g.s.Npad,
                     (int)(2 * g.splits), k);
}

}  // namespace

extern "C" {

size_t hpvg_patchknn_self_ws_bytes(int T, int H, int W, const int* patch, const int* stride, int k) {
  KnnGeom g;
  if (!knn_geom(g, T, H, W, patch, stride, k)) return 0;
  return g.bytes;
}

int hpvg_patchknn_self_u8(const unsigned char* vol, int T, int H, int W, const int* patch, const int* stride, int k, int* kth, void* ws,
                          size_t ws_bytes, void* stream) {
  KnnGeom g;
  if (!vol || !kth || !knn_geom(g, T, H, W, patch, stride, k)) return HPVG_ERR_ARG;
  if (!ws || ws_bytes < g.bytes || ((uintptr_t)ws & 15)) return HPVG_ERR_WORKSPACE;
  signed char* mat = (signed char*)ws + g.off_mat;
  int* norms = (int*)((char*)ws + g.off_norms);
  int* parts = (int*)((char*)ws + g.off_parts);
  hipStream_t st = (hipStream_t)stream;
  pnn_pack_side(vol, mat, norms, nullptr, g.s, nullptr, g.s.N, g.s.Npad, g.p, st);
  if (g.KC == 4) knn_launch<4>(g, mat, norms, parts, kth, k, st);
  else knn_launch<8>(g, mat, norms, parts, kth, k, st);
  return hpvg_launch_status();
}

size_t hpvg_patch_ball_count_ws_bytes(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride,
                                      const int* rstride) {
  PnnGeom g;
  if (!pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, qstride, rstride)) return 0;
  return g.off_keys;  // both packed matrices and their norms; no merge keys
}

int hpvg_patch_ball_count_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr,
                             const int* patch, const int* qstride, const int* rstride, const int* ref_radius, int* count, void* ws,
                             size_t ws_bytes, void* stream) {
  PnnGeom g;
  if (!q || !r || !ref_radius || !count || ((uintptr_t)count & 3) || !pnn_geom(g, Tq, Hq, Wq, Tr, Hr, Wr, patch, qstride, rstride))
    return HPVG_ERR_ARG;
  if (!ws || ws_bytes < g.off_keys || ((uintptr_t)ws & 15)) return HPVG_ERR_WORKSPACE;
  const PnnWs w = pnn_ws(g, ws);  // w.keys is not part of this workspace
  hipStream_t st = (hipStream_t)stream;
  pnn_pack_side(q, w.qmat, w.qn, nullptr, g.q, nullptr, g.mq, g.mqpad, g.p, st);
  pnn_pack_side(r, w.rmat, w.rn, nullptr, g.r, nullptr, g.mr, g.mrpad, g.p, st);
  size_t zblocks = ((size_t)g.q.N / 4 + 255) / 256 + 1;
  if (zblocks > 8192) zblocks = 8192;
  hipLaunchKernelGGL(patchproj_zero_kernel, dim3((unsigned)zblocks), dim3(256), 0, st, count, (size_t)g.q.N);
  long splits, per;
  const long nrt = g.mqpad / PNN_TILE, nct = g.mrpad / PNN_TILE;
  pnn_splits(nrt, nct, splits, per);
  hipLaunchKernelGGL(patchnn_ball_count_kernel, dim3((unsigned)nrt, (unsigned)splits), dim3(256), 0, st, w.qmat, w.rmat, w.qn, w.rn,
                     ref_radius, count, g.q.N, g.r.N, g.p.Dp, (int)nct, (int)per);
  return hpvg_launch_status();
}

}  // extern "C"
