// hp-vae-gan_amd - host-only helpers shared by the convolution launchers (conv_mfma.hip, conv_wgrad.hip).
#pragma once
#include "hpvg_common.h"

// One plan memo per Value type, thread-local, keyed by the seven integers of a launch: open addressing over NSLOT slots of
// which at most half are filled (past that a value is searched per call and handed out from `spill`).  An entry is valid
// while its generation is the caller's: a new generation drops every entry at once without touching the table.
template <class Value, class Search>
const Value& memo_lookup(int gen, int B, int Cin, int Cout, int T, int H, int W, int KT, Search search) {
  struct Entry { int k[7]; int gen; Value v; };
  constexpr int NSLOT = 2048;
  static thread_local Entry cache[NSLOT];
  static thread_local Value spill;
  static thread_local int filled = 0, cur = 0;
  if (cur != gen + 1) {       // (0: an entry never written)
    cur = gen + 1;
    filled = 0;
  }
  unsigned h = 2166136261u;
  for (int v : {B, Cin, Cout, T, H, W, KT}) h = (h ^ (unsigned)v) * 16777619u;
  for (int probe = 0; probe < NSLOT; ++probe) {
    Entry& e = cache[(h + probe) & (NSLOT - 1)];
    if (e.gen != cur) {
      if (filled >= NSLOT / 2) break;
      e = Entry{{B, Cin, Cout, T, H, W, KT}, cur, search()};
      ++filled;
      return e.v;
    }
    const int* c = e.k;
    if (c[0] == B && c[1] == Cin && c[2] == Cout && c[3] == T && c[4] == H && c[5] == W && c[6] == KT) return e.v;
  }
  spill = search();
  return spill;
}

// one launch with up to 160 KB of dynamic LDS: the attribute is set once per kernel instance
template <auto Kernel, class... Args>
int launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args&... a) {
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      (void)hipGetLastError();
    attr = true;
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, a...);
  return hpvg_launch_status();
}
