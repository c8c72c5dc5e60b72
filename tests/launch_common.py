"""What the launch suites share (tests/test_conv_launches.py, tests/test_baseline_conv_launches.py,
tests/test_baseline_ew_launches.py): the checked comparison that keeps the worst ratio per (quantity, kernel kind), the
decoder of the convs' 1-bit mask words, the one-entry cache of a group's inputs and references, and the poisoned-workspace
rerun."""
import torch

import conv_ref as R


def checked(stats, got, ref, A, what, quantity, kind, **kw):
    """conv_ref.check, with the worst |got - ref| / A kept in stats[(quantity, kind)]."""
    r = R.check(got, ref, A, what, **kw)
    k = (quantity, kind)
    stats[k] = max(stats.get(k, 0.0), r)
    return r


def decode_bits(bits, B, C, S, device="cpu"):
    """[B][ceil(C/32)][S] int32 mask words -> bool [B][C][S] on `device`: bit c % 32 of word c / 32."""
    mt = (C + 31) // 32
    assert bits.numel() == B * mt * S
    words = bits.view(B, mt, 1, S).to(device)
    sh = torch.arange(32, dtype=torch.int32, device=device).view(1, 1, 32, 1)
    return ((words >> sh) & 1).view(B, mt * 32, S)[:, :C].bool()


class GroupCache(dict):
    """Inputs and references of ONE group at a time: `get_group(key, make)` returns the cached dict when the key is the
    current one, else drops everything, calls make() and keeps its result."""

    def get_group(self, key, make):
        if self.get("key") == key:
            return self
        self.clear()
        self.update(make())
        self["key"] = key
        return self


def fill_workspaces(ops):
    """Every workspace byte 0xFF (NaN as fp32): a launch that reads a slot it did not write itself cannot reproduce."""
    for buf in ops._ws_cache.values():
        buf.fill_(0xFF)


def assert_same(first, second, tag):
    for k, v in first.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(second[k], v), tag + "%s differs after the workspace was filled with 0xFF" % k


def print_stats(stats, title):
    if stats:
        print("\n" + title)
        for (q, k), v in sorted(stats.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
            print("  %-22s %-14s %.3e" % (q, k, v))
