"""The tap-generic conv launches on tensors at every 4-byte offset, inside the guard bands of tests/offset_buf.py: inputs
surrounded by NaN, outputs and their surroundings preset to a sentinel.  A launch must leave the guards bit-intact, store
every output element, read no NaN - and give the bits it gives on fresh, 256-byte aligned allocations (the kernels have one
dword-wide access form, so the start changes nothing).  On the two smallest shapes of tests/test_conv_taps_launches.py: a
volume smaller than the halo on every axis, where every tap of every output reaches outside the tensor."""
import pytest
import torch

import conv_taps_ref as R
import offset_buf as OB

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(1, 5, 7, 1, 1, 1), (2, 3, 16, 2, 3, 4)]


def _fwd_into(y, x, w, bias, lrelu, mask, flip):
    from hp_vae_gan_amd import ops
    from hp_vae_gan_amd.lib import call, ptr, stream
    K = w.shape[2]
    cin, cout = (w.shape[0], w.shape[1]) if flip else (w.shape[1], w.shape[0])
    g = R.geo(x.shape, cin, cout, K)
    ws = ops._scratch(call("hpvg_convk_fwd_ws_bytes", *g), x.device)
    call("hpvg_convk_fwd_f32", ptr(x), ptr(w), ptr(bias), ptr(y), 1 if lrelu else 0, ptr(mask), 1 if flip else 0, *ws, *g, stream())
    return y


def _wgrad_into(dw, dy, x, accumulate):
    from hp_vae_gan_amd import ops
    from hp_vae_gan_amd.lib import call, ptr, stream
    g = R.geo(x.shape, dw.shape[1], dw.shape[0], dw.shape[2])
    ws = ops._scratch(call("hpvg_convk_bwd_weight_ws_bytes", *g), x.device)
    call("hpvg_convk_bwd_weight_f32", ptr(dy), ptr(x), ptr(dw), 1 if accumulate else 0, *ws, *g, stream())
    return dw


@pytest.mark.parametrize("off", OB.OFFSETS)
@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
@pytest.mark.parametrize("K,dims", [(5, 3), (5, 2), (7, 3), (7, 2)])
def test_launches_at_offsets_inside_guard_bands(K, dims, case, off):
    x, w, b, dy = R.make_case(case, K, dims)
    g = torch.Generator().manual_seed(9)
    my = torch.rand(dy.shape, generator=g) - 0.5
    mx = torch.rand(x.shape, generator=g) - 0.5
    base = torch.rand(w.shape, generator=g) - 0.5
    plain = {k: v.to(DEV) for k, v in dict(x=x, w=w, b=b, dy=dy, my=my, mx=mx).items()}
    # every input at residue 4 * off; a second arrangement staggers the residues so that no two tensors share one
    for tag, offs in (("all", {k: off for k in plain}), ("staggered", {k: (off + i) % 4 for i, k in enumerate(plain)})):
        emb = {k: OB.embed(v, offs[k]) for k, v in plain.items()}
        oo = (off + 1) % 4 if tag == "staggered" else off
        what = "K=%d %dd %s off=%d %s " % (K, dims, case, off, tag)
        # forward with everything the epilogue can read
        y = _fwd_into(OB.out_like(dy.shape, torch.float32, oo, device=DEV), emb["x"], emb["w"], emb["b"], True, emb["my"], False)
        OB.assert_written(y, what + "fwd")
        want = _fwd_into(torch.empty(dy.shape, device=DEV), plain["x"], plain["w"], plain["b"], True, plain["my"], False)
        assert torch.equal(y, want), what + "fwd: the result depends on where the tensors start"
        # backward-data
        dx = _fwd_into(OB.out_like(x.shape, torch.float32, oo, device=DEV), emb["dy"], emb["w"], None, False, emb["mx"], True)
        OB.assert_written(dx, what + "bwd_data")
        want = _fwd_into(torch.empty(x.shape, device=DEV), plain["dy"], plain["w"], None, False, plain["mx"], True)
        assert torch.equal(dx, want), what + "bwd_data: the result depends on where the tensors start"
        # weight gradient, fresh and accumulated (the accumulated form READS its output: it arrives embedded in NaN)
        dw = _wgrad_into(OB.out_like(w.shape, torch.float32, oo, device=DEV), emb["dy"], emb["x"], False)
        OB.assert_written(dw, what + "wgrad")
        want = _wgrad_into(torch.empty(w.shape, device=DEV), plain["dy"], plain["x"], False)
        assert torch.equal(dw, want), what + "wgrad: the result depends on where the tensors start"
        acc = _wgrad_into(OB.embed(base.to(DEV), oo), emb["dy"], emb["x"], True)
        assert OB.guards_intact(acc) and not bool(torch.isnan(acc).any()), what + "wgrad accumulate"
        want = _wgrad_into(base.to(DEV), plain["dy"], plain["x"], True)
        assert torch.equal(acc, want), what + "wgrad accumulate: the result depends on where the tensors start"
        for k, v in emb.items():
            assert OB.guards_intact(v) and torch.equal(v, plain[k]), what + "input %s was written" % k
    # and the aligned result is the right one
    y64, A = R.conv_fwd64(x, w, b)
    R.check(want_fwd(plain), R.lrelu(y64) * torch.where(my > 0, 1.0, 0.2).double(), A, "fwd at offsets")


def want_fwd(plain):
    return _fwd_into(torch.empty(plain["dy"].shape, device=DEV), plain["x"], plain["w"], plain["b"], True, plain["my"], False)
