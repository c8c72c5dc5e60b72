"""Host checks (no GPU) of the tap-generic conv family: the four hpvg_convk_* entry points in the header and the library,
their refusals and workspace sizes, the modules' acceptance of ker_size 5 / 7 (state_dicts of the reference load strictly),
the refusals of paddings, baselines, row slabs and programs, and the float64 references of tests/conv_taps_ref.py with the
seeded defects the tolerance must reject."""
import ctypes

import pytest
import torch

import conv_taps_ref as R
from helpers import hip_opt, load_golden

ENTRY_POINTS = ("hpvg_convk_fwd_ws_bytes", "hpvg_convk_fwd_f32", "hpvg_convk_bwd_weight_ws_bytes", "hpvg_convk_bwd_weight_f32")
OK, ERR_ARG, ERR_WS = 0, -1, -2
FIXTURES = ("taps5_3d_gan_s3.pt", "taps5_3d_vae_s1.pt", "taps5_2d_gan_s2.pt", "taps7_2d_gan_s2.pt")


@pytest.fixture(scope="module")
def lib():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


def test_header_declares_the_entry_points(lib):
    from hp_vae_gan_amd import lib as hplib
    sigs = hplib._SIGNATURES
    for name in ENTRY_POINTS:
        assert name in sigs, name
        assert hasattr(lib, name), name
    assert sigs["hpvg_convk_fwd_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 8)
    assert sigs["hpvg_convk_bwd_weight_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 8)
    P, I = ctypes.c_void_p, ctypes.c_int
    assert sigs["hpvg_convk_fwd_f32"] == (I, [P, P, P, P, I, P, I, P, ctypes.c_size_t] + [I] * 8 + [P])
    assert sigs["hpvg_convk_bwd_weight_f32"] == (I, [P, P, P, I, P, ctypes.c_size_t] + [I] * 8 + [P])


def test_m_tile_switch(lib):
    """hpvg_convk_fwd_mt_config (host only): 0 by size, 1 / 2 forced; anything else is a query."""
    from hp_vae_gan_amd import lib as hplib
    assert hplib._SIGNATURES["hpvg_convk_fwd_mt_config"] == (ctypes.c_int, [ctypes.c_int])
    assert lib.hpvg_convk_fwd_mt_config(-1) == 0
    try:
        for mode in (1, 2, 0, 2):
            assert lib.hpvg_convk_fwd_mt_config(mode) == mode
            assert lib.hpvg_convk_fwd_mt_config(-1) == mode and lib.hpvg_convk_fwd_mt_config(3) == mode
            # the workspace holds the pack of both forms: its size does not follow the switch
            assert lib.hpvg_convk_fwd_ws_bytes(2, 16, 72, 3, 9, 11, 5, 5) == 4 * 125 * 8 * 64 * 4
    finally:
        assert lib.hpvg_convk_fwd_mt_config(0) == 0


# a pointer value that is never dereferenced: every call below is refused on the host, before any launch
FAKE = ctypes.c_void_p(0x1000)
GOOD = dict(B=2, Cin=3, Cout=16, T=3, H=6, W=9, KT=5, K=5)


def _geo(**kw):
    g = dict(GOOD, **kw)
    return [g[k] for k in ("B", "Cin", "Cout", "T", "H", "W", "KT", "K")]


def _fwd(lib, x=FAKE, w=FAKE, y=FAKE, ws=FAKE, ws_bytes=1 << 40, **kw):
    return lib.hpvg_convk_fwd_f32(x, w, None, y, 0, None, 0, ws, ws_bytes, *_geo(**kw), None)


def _wgrad(lib, dy=FAKE, x=FAKE, dw=FAKE, ws=FAKE, ws_bytes=1 << 40, **kw):
    return lib.hpvg_convk_bwd_weight_f32(dy, x, dw, 0, ws, ws_bytes, *_geo(**kw), None)


BAD_GEOMETRY = [dict(K=4, KT=4), dict(K=9, KT=9), dict(K=1, KT=1), dict(K=0, KT=0), dict(K=5, KT=3), dict(K=7, KT=5), dict(K=5, KT=0),
                dict(B=0), dict(Cin=0), dict(Cout=0), dict(T=0), dict(H=0), dict(W=0), dict(B=-1), dict(KT=1, T=2)]


@pytest.mark.parametrize("bad", BAD_GEOMETRY, ids=[",".join("%s=%d" % kv for kv in b.items()) for b in BAD_GEOMETRY])
def test_bad_geometry_is_refused(lib, bad):
    assert _fwd(lib, **bad) == ERR_ARG
    assert _wgrad(lib, **bad) == ERR_ARG
    assert lib.hpvg_convk_fwd_ws_bytes(*_geo(**bad)) == 0
    assert lib.hpvg_convk_bwd_weight_ws_bytes(*_geo(**bad)) == 0


def test_null_tensors_are_refused(lib):
    for name in ("x", "w", "y"):
        assert _fwd(lib, **{name: None}) == ERR_ARG, name
    for name in ("dy", "x", "dw"):
        assert _wgrad(lib, **{name: None}) == ERR_ARG, name


@pytest.mark.parametrize("K,KT,T", [(3, 3, 3), (3, 1, 1), (5, 5, 3), (5, 1, 1), (7, 7, 2), (7, 1, 1)])
def test_workspace_refusals(lib, K, KT, T):
    """null, misaligned (16 bytes, as every workspace of the library) or one byte short: HPVG_ERR_WORKSPACE, after the argument
    checks (a bad argument with a bad workspace is an argument error)."""
    geo = dict(K=K, KT=KT, T=T)
    for call, size in ((_fwd, lib.hpvg_convk_fwd_ws_bytes), (_wgrad, lib.hpvg_convk_bwd_weight_ws_bytes)):
        need = size(*_geo(**geo))
        assert need > 0
        assert call(lib, ws=None, **geo) == ERR_WS
        assert call(lib, ws=None, ws_bytes=0, **geo) == ERR_WS
        for off in (4, 8, 12):
            assert call(lib, ws=ctypes.c_void_p(0x1000 + off), **geo) == ERR_WS
        assert call(lib, ws_bytes=need - 1, **geo) == ERR_WS
        assert call(lib, ws_bytes=0, **geo) == ERR_WS
        assert call(lib, ws=None, **dict(geo, B=0)) == ERR_ARG


def test_workspace_sizes_are_positive_and_monotone(lib):
    for size in (lib.hpvg_convk_fwd_ws_bytes, lib.hpvg_convk_bwd_weight_ws_bytes):
        for K in (3, 5, 7):
            for KT in (1, K):
                base = dict(B=1, Cin=1, Cout=1, T=1 if KT == 1 else 2, H=1, W=1, K=K, KT=KT)
                assert size(*_geo(**base)) > 0
                # the channel counts: more channels never need less
                prev = 0
                for C in (1, 2, 3, 5, 16, 31, 32, 33, 64, 65, 72, 128):
                    n = size(*_geo(**dict(base, Cin=C, Cout=C)))
                    assert n >= prev and n > 0, (K, KT, C)
                    prev = n
                for key in ("Cin", "Cout"):
                    assert size(*_geo(**dict(base, **{key: 64}))) >= size(*_geo(**dict(base, **{key: 8})))
        # the tap side and the tap count: 7 > 5 > 3, 3-D > 2-D
        a = [size(*_geo(B=2, Cin=16, Cout=16, T=1, H=9, W=11, KT=1, K=K)) for K in (3, 5, 7)]
        assert a[0] < a[1] < a[2], a
        for K in (3, 5, 7):     # (T = 1 on both sides: the same volume with K x K and with K x K x K taps)
            assert size(*_geo(B=2, Cin=16, Cout=16, T=1, H=9, W=11, KT=1, K=K)) < size(*_geo(B=2, Cin=16, Cout=16, T=1, H=9, W=11, KT=K, K=K))
    # the forward's workspace is the packed weight: it does not depend on the volume, and covers every weight element
    for K in (3, 5, 7):
        sizes = {lib.hpvg_convk_fwd_ws_bytes(B, 16, 24, T, H, W, K, K) for B, T, H, W in ((1, 1, 1, 1), (2, 3, 9, 11), (4, 13, 144, 256))}
        assert len(sizes) == 1 and sizes.pop() >= 16 * 24 * K ** 3 * 4
    # the weight gradient's holds at least one partial weight, and more position tiles never need less
    for K in (3, 5, 7):
        prev = 0
        for B, T, H, W in ((1, 1, 1, 1), (1, 2, 5, 9), (2, 3, 9, 11), (2, 4, 30, 40), (4, 13, 144, 256)):
            n = lib.hpvg_convk_bwd_weight_ws_bytes(B, 16, 24, T, H, W, K, K)
            assert n >= 16 * 24 * K ** 3 * 4 and n >= prev and n % 16 == 0
            prev = n


# ------------------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("fname", FIXTURES)
def test_reference_state_dicts_load_strictly(fname):
    from hp_vae_gan_amd.modules import networks_2d, networks_3d
    fx = load_golden(fname)
    K = fx["opt"]["ker_size"]
    assert K in (5, 7) and fx["opt"]["padd_size"] == K // 2
    nets = networks_3d if fx["dims"] == 3 else networks_2d
    opt = hip_opt(fx["opt"], fx["dims"], fx["scale_idx"], "cpu")
    netG = nets.GeneratorHPVAEGAN(opt)
    for _ in range(fx["scale_idx"]):
        netG.init_next_stage()
    # names, shapes and ORDER are the reference's
    assert [(k, tuple(v.shape)) for k, v in netG.state_dict().items()] == [(k, tuple(v.shape)) for k, v in fx["G_init"].items()]
    netG.load_state_dict(fx["G_init"], strict=True)
    assert tuple(netG.decoder.head.conv.weight.shape[2:]) == (K,) * fx["dims"]
    if fx["D_init"] is not None:
        netD = getattr(nets, opt.discriminator)(opt)
        assert [(k, tuple(v.shape)) for k, v in netD.state_dict().items()] == [(k, tuple(v.shape)) for k, v in fx["D_init"].items()]
        netD.load_state_dict(fx["D_init"], strict=True)
        assert netD.tail.ker_size == K and netD.tail.padding == 1     # the critic's tail shrinks its output (crop K // 2 - 1)


def test_seeded_construction_draws_like_torch():
    """Parameter initialisers run in nn.ConvNd's / spectral_norm's order, so a seeded construction equals torch's own."""
    import torch.nn as nn
    from hp_vae_gan_amd.modules import _nets
    for K, dims in ((5, 3), (7, 2)):
        torch.manual_seed(5)
        ours = _nets.Conv(dims, 3, 4, K, K // 2, 1)
        torch.manual_seed(5)
        ref = (nn.Conv3d if dims == 3 else nn.Conv2d)(3, 4, K, 1, K // 2)
        assert torch.equal(ours.weight, ref.weight) and torch.equal(ours.bias, ref.bias)
        torch.manual_seed(6)
        sn = _nets.SNConv(dims, 3, 4, K, K // 2, 1)
        torch.manual_seed(6)
        rsn = nn.utils.spectral_norm((nn.Conv3d if dims == 3 else nn.Conv2d)(3, 4, K, 1, K // 2))
        for k, v in rsn.state_dict().items():
            assert torch.equal(sn.state_dict()[k], v), k
        assert list(sn.state_dict()) == list(rsn.state_dict())


def test_padding_rules():
    from hp_vae_gan_amd.modules import _nets
    for K in (5, 7):
        for p in range(K // 2 + 1):
            _nets.Conv(3, 2, 2, K, p, 1)
            _nets.SNConv(2, 2, 2, K, p, 1)
        for cls in (_nets.Conv, _nets.SNConv):
            for bad in (dict(padding=K // 2 + 1), dict(padding=-1), dict(stride=2)):
                kw = dict(dict(padding=K // 2, stride=1), **bad)
                with pytest.raises(NotImplementedError, match=r"ker_size in \{5, 7\} with 0 <= padding <= ker_size // 2"):
                    cls(3, 2, 2, K, kw["padding"], kw["stride"])
    for K in (2, 4, 6, 9):
        with pytest.raises(NotImplementedError, match="ker_size"):
            _nets.Conv(3, 2, 2, K, K // 2, 1)
    # ker_size 1 and 3 are what they were
    _nets.Conv(3, 2, 2, 3, 0, 1), _nets.Conv(3, 2, 2, 3, 1, 1), _nets.Conv(3, 2, 2, 1, 0, 1), _nets.SNConv(3, 2, 2, 3, 1, 1)
    with pytest.raises(NotImplementedError):
        _nets.SNConv(3, 2, 2, 3, 0, 1)
    with pytest.raises(NotImplementedError):
        _nets.Conv(3, 2, 2, 3, 2, 1)


def test_a_crop_that_empties_the_volume_is_refused_by_name():
    from hp_vae_gan_amd.modules import _nets
    y = torch.zeros(1, 1, 4, 2, 9)
    with pytest.raises(ValueError, match=r"Conv\(8 -> 1\): ker_size=5 with padding=1 leaves nothing of a 4x2x9 input"):
        _nets.crop_wide(y, 5, 1, "Conv(8 -> 1)")
    with pytest.raises(ValueError, match=r"ker_size=7 with padding=1 leaves nothing of a 4x9 input"):
        _nets.crop_wide(torch.zeros(1, 1, 4, 9), 7, 1, "Conv(8 -> 1)")
    assert _nets.crop_wide(y, 5, 2, "same") is y


def _baseline_opt(**kw):
    import types
    return types.SimpleNamespace(**dict(dict(nfc=4, nc_im=3, num_layer=3, ker_size=5, padd_size=2), **kw))


@pytest.mark.parametrize("name", ["GeneratorSG", "GeneratorCSG", "WDiscriminatorBaselines"])
def test_baselines_refuse_other_tap_sides(name):
    from hp_vae_gan_amd.modules import networks_3d
    with pytest.raises(NotImplementedError, match=name + r".*pads of num_layer \+ 2 voxels fit ker_size=3 only.*got ker_size=5"):
        getattr(networks_3d, name)(_baseline_opt())
    getattr(networks_3d, name)(_baseline_opt(ker_size=3, padd_size=1))


def test_row_slabs_refuse_wide_taps_before_any_work():
    from hp_vae_gan_amd import multigpu
    from hp_vae_gan_amd.modules import networks_3d
    fx = load_golden("taps5_3d_gan_s3.pt")
    opt = hip_opt(fx["opt"], 3, fx["scale_idx"], "cpu")
    netG = networks_3d.GeneratorHPVAEGAN(opt)
    netG.init_next_stage()
    netD = networks_3d.WDiscriminator3D(opt)

    class Plan:
        halo = object()

        def covers(self, level):
            return True

    with pytest.raises(NotImplementedError, match=r"row slabs \(8-rank mode\).*ker_size=5 > 3"):
        multigpu.HipBackend.set_slab(None, netG, netD, Plan())
    assert netG.slab is None
    assert all(m.halo is None for net in (netG, netD) for m in net.modules() if hasattr(m, "halo"))
    multigpu.HipBackend.set_slab(None, netG, netD, None)     # taking slabs off stays possible


def test_programs_refuse_at_start_up(tmp_path):
    from hp_vae_gan_amd import programs, train_image, train_video, train_video_baselines
    programs.check_tap_flags(3, 1), programs.check_tap_flags(3, 0), programs.check_tap_flags(1, 0)
    programs.check_tap_flags(5, 2), programs.check_tap_flags(7, 3)
    for K, p in ((5, 1), (5, 0), (5, 3), (7, 1), (7, 2)):
        with pytest.raises(SystemExit, match=r"--ker-size %d needs --padd-size ker_size // 2 = %d \(got %d\)" % (K, K // 2, p)):
            programs.check_tap_flags(K, p)
    for K in (2, 4, 6, 9):
        with pytest.raises(SystemExit, match="--ker-size %d: the convolutions run 3, 5 or 7 taps" % K):
            programs.check_tap_flags(K, K // 2)
    clip = str(tmp_path / "clip.npy")
    # the refusal comes before the data and the device are looked at: the clip does not exist, and there may be no GPU
    with pytest.raises(SystemExit, match=r"--padd-size ker_size // 2 = 2"):
        train_video.main(["--video-path", clip, "--ker-size", "5", "--run-dir", str(tmp_path)])
    with pytest.raises(SystemExit, match=r"--padd-size ker_size // 2 = 3"):
        train_image.main(["--image-path", clip, "--ker-size", "7", "--padd-size", "2", "--run-dir", str(tmp_path)])
    with pytest.raises(SystemExit, match=r"--ker-size 5: the SinGAN baselines' hard-wired pads .* fit ker_size=3 only"):
        train_video_baselines.main(["--video-path", clip, "--ker-size", "5", "--padd-size", "2", "--run-dir", str(tmp_path)])
    assert list(tmp_path.iterdir()) == []


def test_ops_decides_by_the_tap_side():
    from hp_vae_gan_amd import ops
    assert ops._side((4, 3, 5, 5, 5)) == 5 and ops._kt((4, 3, 5, 5, 5)) == 5
    assert ops._side((4, 3, 7, 7)) == 7 and ops._kt((4, 3, 7, 7)) == 1
    assert ops._side((4, 3, 3, 3, 3)) == 3 and ops._kt((4, 3, 3, 3, 3)) == 3 and ops._kt((4, 3, 3, 3)) == 1
    for bad in ((4, 3, 5, 5, 3), (4, 3, 3, 5), (4, 3, 4, 4), (4, 3, 9, 9, 9), (4, 3, 1, 1), (4, 3, 5)):
        with pytest.raises(RuntimeError):
            ops._side(bad)


# --------------------------------------------------------------------------------------------------------- references
CASES = [((2, 3, 4, 3, 4, 5), 5, 3), ((1, 4, 3, 1, 6, 7), 5, 2), ((1, 2, 3, 1, 5, 8), 7, 2), ((1, 3, 2, 2, 3, 4), 7, 3), ((2, 3, 4, 3, 4, 5), 3, 3)]


@pytest.mark.parametrize("case,K,dims", CASES)
def test_references_equal_plain_sums_over_taps(case, K, dims):
    x, w, b, dy = R.make_case(case, K, dims)
    x64, w64, d64 = x.double(), w.double(), dy.double()
    y, A = R.conv_fwd64(x, w)
    assert torch.allclose(y, R.fwd_taps(x64, w64), rtol=0, atol=1e-13)
    assert torch.allclose(A.double(), R.fwd_taps(x64.abs(), w64.abs()), rtol=1e-6, atol=0)
    yb, Ab = R.conv_fwd64(x, w, b)
    assert torch.allclose(yb, y + b.double().view(1, -1, *([1] * dims)), rtol=0, atol=1e-13) and bool((Ab >= A).all())
    dx, Ad = R.conv_bwd_data64(dy, w)
    assert torch.allclose(dx, R.bwd_data_taps(d64, w64), rtol=0, atol=1e-13)
    assert torch.allclose(Ad.double(), R.bwd_data_taps(d64.abs(), w64.abs()), rtol=1e-6, atol=0)
    dw, Aw = R.conv_bwd_weight64(dy, x, w.shape)
    assert torch.allclose(dw, R.bwd_weight_taps(d64, x64, K), rtol=0, atol=1e-12)
    assert torch.allclose(Aw.double(), R.bwd_weight_taps(d64.abs(), x64.abs(), K), rtol=1e-6, atol=0)
    # and against autograd of the padded conv
    xr, wr = x64.clone().requires_grad_(True), w64.clone().requires_grad_(True)
    conv = torch.nn.functional.conv3d if dims == 3 else torch.nn.functional.conv2d
    gx, gw = torch.autograd.grad(conv(xr, wr, padding=K // 2), (xr, wr), d64)
    assert torch.allclose(dx, gx, rtol=0, atol=1e-13) and torch.allclose(dw, gw, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case,K,dims", CASES[:4])
def test_seeded_defects_are_rejected_at_the_tolerance(case, K, dims):
    """What the per-element bound must catch: one tap 1 % off, a flip that forgets to reverse the taps, a halo of h - 1.  A
    correct fp32 evaluation passes the same check."""
    x, w, b, dy = R.make_case(case, K, dims)
    x64, w64, d64 = x.double(), w.double(), dy.double()
    y, A = R.conv_fwd64(x, w)
    dx, Ad = R.conv_bwd_data64(dy, w)
    dw, Aw = R.conv_bwd_weight64(dy, x, w.shape)
    conv = torch.nn.functional.conv3d if dims == 3 else torch.nn.functional.conv2d
    assert R.err_ratio(conv(x, w, padding=K // 2), y, A)[0] <= R.TAU / 10           # fp32 on the CPU: well inside
    # one tap 1 % off (the centre's neighbour along W: a volume smaller than the halo still reaches it)
    w_bad = w64.clone()
    w_bad[(0, 0) + (K // 2,) * (dims - 1) + (K // 2 - 1,)] *= 1.01
    assert R.err_ratio(R.fwd_taps(x64, w_bad), y, A)[0] > R.TAU
    w_bad = w64.clone()
    w_bad[(-1, -1) + (K // 2,) * (dims - 1) + (K // 2 + 1,)] *= 1.01
    assert R.err_ratio(R.bwd_data_taps(d64, w_bad), dx, Ad)[0] > R.TAU
    dw_bad = dw.clone()
    dw_bad[(0, 0) + (K // 2,) * dims] *= 1.01
    assert R.err_ratio(dw_bad, dw, Aw)[0] > R.TAU
    # the flip without the tap reversal
    assert R.err_ratio(R.bwd_data_taps(d64, w64, reverse=False), dx, Ad)[0] > R.TAU
    # a halo of h - 1
    assert R.err_ratio(R.fwd_taps(x64, w64, halo=K // 2 - 1), y, A)[0] > R.TAU
    assert R.err_ratio(R.fwd_taps(x64, w64, halo=K // 2), y, A)[0] < 1e-12     # (float64 in another summation order)
