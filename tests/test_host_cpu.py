"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol of include/hpvg.h, the pyramid
tables of the product package equal the reference's (golden tables.json), module trees / state_dict layouts accept
the reference's state_dicts, Adam parameter groups follow train_video.py:57-86, and compute on CPU fails loudly."""
import ctypes
import json
import os
import re

import pytest
import torch

import hp_vae_gan_amd as hp
from hp_vae_gan_amd import lib as hplib
from hp_vae_gan_amd import train as hp_train
from hp_vae_gan_amd import utils as hu
from hp_vae_gan_amd.modules import networks_2d, networks_3d
from helpers import GOLDEN, load_golden, opt_from
from oracle import hpvg_oracle as O


def test_library_loads_and_exports_header_symbols():
    declared = hplib.check_symbols()
    assert len(declared) >= 35
    lib = ctypes.CDLL(hplib.LIB_PATH)
    for s in declared:
        assert hasattr(lib, s), s


def test_header_signatures_frozen():
    """Declarations that between them use every C type of include/hpvg.h, as the parser must bind them."""
    c = ctypes
    P, I, L, F, D, Z = c.c_void_p, c.c_int, c.c_long, c.c_float, c.c_double, c.c_size_t
    want = {
        "hpvg_bn_finalize_f32": ([P, D, P, P, P, P, F, F, P, P, P, P, I, P], I),
        "hpvg_normal_f32": ([P, L, c.c_ulonglong, c.c_uint, P, P], I),
        "hpvg_scalar_log_append_f32": ([hplib.ScalarPtrs, I, P, I, P, P], I),
        "hpvg_hist_w1_i32": ([P, L, P, L, I, L, P, P], I),
        "hpvg_sn_power_iter_batch_f32": ([I] + [P] * 8 + [I, F, P, Z, P], I),    # pointer-to-pointer parameters
        "hpvg_clip_scale_f32": ([P, L, P, F, P, P], I),                          # a comment inside the parameter list
        "hpvg_reduce_ws_bytes": ([], Z),
        "hpvg_patchproj_bins": ([P], Z),
        "hpvg_conv_wino_config": ([I, L], I),
    }
    with open(hplib.HEADER_PATH) as f:
        sigs, _ = hplib.parse_header(f.read())
    for name, (args, ret) in want.items():
        assert sigs[name] == (ret, args), name


def test_every_declaration_is_parsed_and_bound():
    with open(hplib.HEADER_PATH) as f:
        text = f.read()
    sigs, _ = hplib.parse_header(text)
    names = set(re.findall(r"\b(hpvg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert names == set(sigs) and sorted(names) == hplib.check_symbols()
    lib = hplib.load()
    for name, (ret, args) in sigs.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is ret, name
        assert ret in (ctypes.c_int, ctypes.c_size_t), name


@pytest.mark.parametrize("decl", [
    "int hpvg_x(const float* a, short n, void* stream);",            # a scalar type outside the known set
    "int hpvg_x(void (*cb)(int), void* stream);",                    # a function-pointer parameter
    "float hpvg_x(const float* a);",                                 # an unknown return type
    "const char* hpvg_x(int code);",
    "int hpvg_x(int);",                                              # no parameter name: the type cannot be told from it
])
def test_header_parser_refuses_what_it_does_not_understand(decl):
    ok = "#define HPVG_N 4\n/* int hpvg_hidden(short n); */\nsize_t hpvg_ok(int n, /* why */ unsigned long long seed);\n"
    sigs, consts = hplib.parse_header(ok)
    assert sigs == {"hpvg_ok": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_ulonglong])} and consts == {"HPVG_N": 4}
    with pytest.raises(ImportError, match="hpvg_x"):
        hplib.parse_header(ok + decl + "\n")


def test_header_constants():
    from hp_vae_gan_amd import ops
    assert (ops.PACK_BATCH_MAX, hplib.LOG_MAX_K, ops.SN_BATCH_MAX) == (16, 16, 8)
    assert ctypes.sizeof(hplib.ScalarPtrs) == 16 * ctypes.sizeof(ctypes.c_void_p)
    with open(hplib.HEADER_PATH) as f:
        consts = hplib.parse_header(f.read())[1]
    assert consts["HPVG_PACK_BATCH_MAX"] == 16 and consts["HPVG_LOG_MAX_K"] == 16 and consts["HPVG_SN_BATCH_MAX"] == 8
    assert {k: v for k, v in consts.items() if k.startswith("HPVG_ERR_")} == \
        {"HPVG_ERR_ARG": -1, "HPVG_ERR_WORKSPACE": -2, "HPVG_ERR_UNSUPPORTED": -3, "HPVG_ERR_LAUNCH": -4}
    with pytest.raises(RuntimeError, match="hpvg_conv_fwd_plan failed: HPVG_ERR_ARG"):    # call() prints the header's name of the code
        hplib.call("hpvg_conv_fwd_plan", 1, 1, 1, 1, 1, 1, 2, (ctypes.c_int * 10)())


def test_size_queries_and_plans_run_without_gpu():
    # wide layers carry the Winograd U fragments (36 tap-points per chunk + 4 of tail padding) behind the direct pack
    # ... and the 3x3x3 ones the two-axis U fragments behind those ([16 sub-chunks][3 dt][2 channel pairs][4 rows][2 m-tiles][64][4])
    assert hplib.call("hpvg_conv_wpack_floats", 64, 64, 3) == (8 * 27 + 2) * 2 * 64 * 4 + (8 * 36 + 4) * 2 * 64 * 4 + 16 * 3 * 2 * 4 * 2 * 64 * 4
    assert hplib.call("hpvg_conv_wpack_floats", 64, 64, 1) == (8 * 9 + 2) * 2 * 64 * 4 + (8 * 12 + 4) * 2 * 64 * 4
    assert hplib.call("hpvg_conv_wpack_floats", 64, 32, 3) == (8 * 27 + 2) * 1 * 64 * 4     # Cout <= 32: direct kernel only
    assert hplib.call("hpvg_conv_wpack_floats", 3, 64, 3) == (1 * 27 + 2) * 2 * 64 * 2
    out = (ctypes.c_int * 10)()
    for (B, Ci, Co, T, H, W, KT) in [(2, 64, 64, 13, 144, 256, 3), (2, 64, 64, 4, 18, 33, 3), (2, 3, 64, 1, 192, 256, 1), (2, 64, 3, 7, 91, 162, 3)]:
        assert hplib.call("hpvg_conv_fwd_plan", B, Ci, Co, T, H, W, KT, out) == 0
        L, Tw, nrange, ntw, nblocks, NB, MB, gridy, lds, ntiles = list(out)
        # tiles = ranges of L flattened positions (row stride Tw + 2) of a band of Tw columns
        assert L >= 1 and Tw >= 1 and ntw * Tw >= W and nrange * L >= (H - 1) * (Tw + 2) + Tw
        assert nblocks <= 4 * NB and nblocks * 32 >= L and lds <= 160 * 1024
        assert ntiles == B * T * nrange * ntw
        assert hplib.call("hpvg_conv_bwd_weight_plan", B, Ci, Co, T, H, W, KT, out) == 0
        assert out[0] >= 1 and out[8] <= 160 * 1024 and out[5] >= 1
        assert hplib.call("hpvg_conv_bwd_weight_ws_bytes", B, Ci, Co, T, H, W, KT) > 0
    with pytest.raises(RuntimeError, match="HPVG_ERR_ARG"):  # bad KT -> error code, not a crash
        hplib.call("hpvg_conv_fwd_plan", 1, 1, 1, 1, 1, 1, 2, out)
    with pytest.raises(RuntimeError, match="HPVG_ERR_ARG"):  # a dimension below 1 -> error code, not a division by zero
        hplib.call("hpvg_conv_fwd_plan", 0, 64, 64, 4, 18, 33, 3, out)
    assert hplib.load().hpvg_conv_narrow_plan(0, 64, 3, 4, 18, 33, 3, (ctypes.c_int * 55)()) == -1


def test_winograd_conv_plan_geometry():
    """The tile plan of conv_wino_kernel over every width, both staging forms (halo'd bands for odd or very wide images, rows
    as they lie in memory for even widths): even band width and row stride (an output pair never straddles a row or a
    band), even tile length within the accumulator blocks, every output position covered, every LDS read of a lane inside
    the tile buffer, the staged plane within the staging slots / one 16-byte group per lane, every staged group written
    inside the tile buffer."""
    lib = hplib.load()
    out = (ctypes.c_int * 10)()
    assert lib.hpvg_conv_wino_plan(2, 3, 64, 5, 9, 16, 3, out) != 0     # Cin < 8: direct kernel
    assert lib.hpvg_conv_wino_plan(2, 64, 32, 5, 9, 16, 3, out) != 0    # one m-tile: direct kernel
    prev = lib.hpvg_conv_wino_config(-1, -1)
    seen = set()
    try:
        for mode, KT, T in ((3, 3, 5), (3, 1, 1), (1, 3, 5), (4, 3, 5)):   # 3 / 4: one staging form forced, 1: the planner's own pick
            assert lib.hpvg_conv_wino_config(mode, -1) == mode
            for H in (1, 2, 9, 45, 144):
                for W in list(range(1, 70)) + [81, 129, 130, 146, 183, 230, 255, 256, 284, 286, 300, 380, 382, 640]:
                    for Cout in (64, 70, 128):
                        assert lib.hpvg_conv_wino_plan(2, 64, Cout, T, H, W, KT, out) == 0, (KT, H, W)
                        seen.add((mode, out[4] == out[1]))
                        assert mode != 4 or out[4] != out[1]
                        L, Tw, nrange, ntw, RS, NBP, MBW, gridy, lds, ntiles = list(out)
                        assert L % 2 == 0 and 2 <= L <= NBP * 128
                        assert gridy * MBW * 32 >= Cout and ntiles == 2 * T * nrange * ntw * gridy and lds <= 80 * 1024
                        if RS == Tw:
                            # staging form 2: one band of the full (even) width, rows as they lie in memory, 16-byte pieces
                            assert W % 2 == 0 and Tw == W and ntw == 1 and nrange * L >= H * W
                            PL = 2 * W + NBP * 128 + 10
                            assert lds == 8 * KT * PL * 4
                            assert (L + 2 * W + 2 + 6) // 4 <= 256             # one 16-byte group per lane
                            # ... each WRITTEN whole, one float into the plane slot: the last group of the last plane ends
                            # inside the buffer (a group that crosses the end of the workgroup's LDS is dropped by the hardware)
                            assert 1 + 4 * ((L + 2 * W + 2 + 6) // 4) <= PL
                            assert 4 + 2 * (NBP * 64 - 1) + 2 * W + 3 < PL      # furthest read of a lane (image offset <= 4)
                            continue
                        assert Tw % 2 == 0 and RS == Tw + 2
                        assert ntw * Tw >= W and (ntw - 1) * Tw < W
                        assert nrange * L >= (H - 1) * RS + Tw                 # every output position of a band plane
                        PL = NBP * 128 + 2 * RS + 2
                        assert lds == 8 * KT * PL * 4
                        assert L + 2 * RS + 2 <= 1024                          # staged positions per plane
                        # furthest read of a lane: pair NBP*64 - 1, row tap 2, inputs d2 d3
                        assert 2 * (NBP * 64 - 1) + 2 * RS + 3 < PL
    finally:
        lib.hpvg_conv_wino_config(prev, -1)
    assert {(3, True), (3, False), (1, True), (1, False), (4, False)} <= seen   # both forms met, forced and picked


def test_winograd_weight_gradient_plan_geometry():
    """The tile plan of conv_wgradw_kernel: even band width / row stride, channel strides 2 (mod 4) (8-byte pairs of a
    half-wave's 32 channel rows in 32 different bank pairs), every read of the K loop inside its row, two buffers in LDS."""
    lib = hplib.load()
    out = (ctypes.c_int * 10)()
    prev = lib.hpvg_conv_bwd_weight_wino_config(-1)
    try:
        for mode in (2, 3):     # 3: the 4-byte staging form for every width
            assert lib.hpvg_conv_bwd_weight_wino_config(mode) == mode
            for KT, T in ((3, 5), (1, 1)):
                for H in (1, 2, 9, 45, 144):
                    for W in list(range(1, 70)) + [81, 129, 130, 146, 183, 204, 230, 255, 256, 300]:
                        assert lib.hpvg_conv_bwd_weight_wino_plan(2, 64, 64, T, H, W, KT, out) == 0, (KT, H, W)
                        Th, Tw, nth, ntw, QK, S, DS, XS, lds, ntiles = list(out)
                        assert ntw * Tw >= W and (ntw - 1) * Tw < W and nth * Th >= H and (nth - 1) * Th < H
                        assert DS % 4 == 2 and XS % 4 == 2
                        assert lds == 2 * 64 * (DS + XS) * 4 and lds <= 160 * 1024 and DS <= 512 and XS <= 512
                        assert ntiles == 2 * T * nth * ntw and 1 <= S <= 256
                        assert hplib.call("hpvg_conv_bwd_weight_ws_bytes", 2, 64, 64, T, H, W, KT) >= 256 + S * KT * 12 * 4096 * 4
                        if mode == 2 and W % 4 == 0:
                            # 16-byte form: dY rows of Tw floats, X rows of Tw + 8 from column w0 - 4, one float into the
                            # channel row; at most two 64-lane pieces per row and operand
                            assert Tw % 4 == 0 and QK == Th * Tw and DS == QK + 2 and XS == (Th + 2) * (Tw + 8) + 2
                            assert Th * (Tw // 4) <= 128 and (Th + 2) * (Tw // 4 + 2) <= 128
                        else:
                            RS = Tw + 2
                            assert Tw % 2 == 0 and QK % 4 == 0 and QK >= Th * RS
                            assert DS >= QK and XS >= QK + 2 * RS + 2 and XS >= (Th + 2) * RS  # furthest read: QK - 2 + 2*RS + 3
    finally:
        lib.hpvg_conv_bwd_weight_wino_config(prev)


def test_two_axis_weight_gradient_plan_geometry():
    """The tile plan of conv_wgradw2_kernel over every width 1 .. 300 (the kernel takes any: odd widths and W % 4 != 0 through
    the straddle patch): an even tile height, bands of a multiple of 4 columns (never 4 / 8 wide where a wider band fits), an
    even number of K steps (Th * Tw % 16 = 0: the loop body holds two), at most two 64-lane pieces per channel row and operand,
    channel strides 2 (mod 4), every read of the K loop inside its channel row, two buffers in LDS, and the straddling group of
    a W % 4 != 0 row inside the band that stages it."""
    lib = hplib.load()
    out = (ctypes.c_int * 11)()
    for KT, T in ((3, 5), (1, 1)):
        for H in (1, 2, 9, 45, 91, 144):
            for W in range(1, 301):
                assert lib.hpvg_conv_bwd_weight_wino2_plan(2, 64, 64, T, H, W, KT, out) == 0, (KT, H, W)
                Th, Tw, nth, ntw, QK, S, DS, XS, lds, ntiles, wanted = list(out)
                assert Th % 2 == 0 and Tw % 4 == 0 and QK == Th * Tw and QK % 16 == 0
                assert ntw * Tw >= W and (ntw - 1) * Tw < W and nth * Th >= H and (nth - 1) * Th < H + 3
                assert Tw >= 12 or W < 24, (H, W, Tw)
                RS = Tw + 8
                assert DS == QK + 2 and XS == (Th + 2) * RS + 2 and DS % 4 == 2 and XS % 4 == 2
                assert Th * (Tw // 4) <= 128 and (Th + 2) * (Tw // 4 + 2) <= 128
                assert lds == 2 * 64 * (DS + XS) * 4 and lds <= 160 * 1024
                # furthest reads of a step: dY row 1 of the last quad row, X patch row 3 / column pair 1 of the last quad
                assert (Th - 1) * Tw + (Tw - 2) + 1 < DS and (Th + 1) * RS + (Tw - 2) + 4 + 3 < XS
                assert ntiles == 2 * T * nth * ntw and 1 <= S <= 256 and wanted in (0, 1)
                if W % 4:
                    gs = W - W % 4                      # the straddling group lies in the last band's dY rows and X rows
                    w0 = (ntw - 1) * Tw
                    assert 0 <= gs - w0 < Tw and 0 <= gs - (w0 - 4) < Tw + 8
                assert hplib.call("hpvg_conv_bwd_weight_ws_bytes", 2, 64, 64, T, H, W, KT) >= 256 + S * KT * 16 * 4096 * 4
    # the size rule: the stage shapes of the video pyramid that run it by default (B = 2)
    for (T, H, W), want in {(13, 144, 256): 1, (7, 114, 204): 1, (7, 91, 162): 1, (7, 72, 129): 1, (5, 57, 102): 1, (5, 36, 65): 1,
                            (4, 18, 33): 0}.items():
        assert lib.hpvg_conv_bwd_weight_wino2_plan(2, 64, 64, T, H, W, 3, out) == 0 and out[10] == want, (T, H, W, out[10])


def test_tables_match_reference():
    rows = json.load(open(os.path.join(GOLDEN, "tables.json")))
    for row in rows:
        opt = opt_from(dict(min_size=row["min_size"], max_size=row["max_size"], img_size=row["img_size"], ar=row["ar"],
                            scale_factor_init=0.75, sampling_rates=[4, 3, 2, 1], fps_lcm=12, org_fps=24))
        hu.adjust_scales2image(opt.img_size, opt)
        opt.stop_scale_time = opt.stop_scale
        assert (opt.num_scales, opt.stop_scale, opt.scale1, opt.scale_factor) == (row["num_scales"], row["stop_scale"], row["scale1"], row["scale_factor"])
        for lv in row["levels"]:
            i = lv["index"]
            assert hu.get_scales_by_index(i, opt.scale_factor, opt.stop_scale, opt.img_size) == lv["w"]
            fps, td, fi = hu.get_fps_td_by_index(i, opt)
            assert (fps, td, fi) == (lv["fps"], lv["td"], lv["fps_index"])
            assert hu.images.level_shape_3d(i, opt) == [lv["td"], lv["h"], lv["w"]]
            assert hu.images.level_shape_2d(i, opt) == [lv["h"], lv["w"]]


@pytest.mark.parametrize("fname", ["step3d_gan_s3.pt", "step2d_gan_s2.pt"])
def test_state_dict_layout_is_the_references(fname):
    fx = load_golden(fname)
    dims, s = fx["dims"], fx["scale_idx"]
    nets = networks_3d if dims == 3 else networks_2d
    opt = opt_from(fx["opt"])
    G = nets.GeneratorHPVAEGAN(opt)
    for _ in range(s):
        G.init_next_stage()
    assert list(G.state_dict().keys()) == list(fx["G_init"].keys())
    G.load_state_dict(fx["G_init"], strict=True)
    D = (nets.WDiscriminator3D if dims == 3 else nets.WDiscriminator2D)(opt)
    assert list(D.state_dict().keys()) == list(fx["D_init"].keys())
    D.load_state_dict(fx["D_init"], strict=True)
    assert [n for n, _ in G.named_parameters()] == [k for k in fx["G_init"] if O.is_param(k)]
    for k, v in fx["G_init"].items():
        assert G.state_dict()[k].shape == v.shape and G.state_dict()[k].dtype == v.dtype


def test_seeded_construction_consumes_rng_like_reference():
    """Same torch initialisers in the same order: a seeded build reproduces the fixture-independent init statistics."""
    opt = opt_from(dict(nc_im=3, nfc=8, latent_dim=8, enc_blocks=2, ker_size=3, num_layer=5, padd_size=1, vae_levels=2, train_all=False))
    torch.manual_seed(3)
    a = networks_3d.GeneratorHPVAEGAN(opt)
    torch.manual_seed(3)
    b = networks_3d.GeneratorHPVAEGAN(opt)
    for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(x, y), k
    w = a.decoder.head.conv.weight
    bound = 1 / (8 * 27) ** 0.5
    assert float(w.abs().max()) <= bound + 1e-6 and float(a.decoder.head.norm.weight.min()) == 1.0
    u = a.encode.features.conv_block_0.conv.weight_u
    assert abs(float(u.norm()) - 1.0) < 1e-5


def test_param_groups_follow_reference_rules():
    base = dict(nc_im=3, nfc=8, latent_dim=8, enc_blocks=2, ker_size=3, num_layer=5, padd_size=1, lr_g=5e-4, lr_scale=0.2, train_depth=1)
    for vae_levels, scale_idx, train_all in [(3, 0, False), (3, 2, False), (3, 3, False), (3, 5, False), (1, 1, False), (3, 1, True), (3, 4, True)]:
        opt = opt_from(dict(base, vae_levels=vae_levels, scale_idx=scale_idx, train_all=train_all))
        G = networks_3d.GeneratorHPVAEGAN(opt)
        for _ in range(scale_idx):
            G.init_next_stage()
        groups = hp_train.generator_param_groups(opt, G)
        got = []
        names = {id(p): n for n, p in G.named_parameters()}
        for params, lr in groups:
            ps = list(params)
            prefix = os.path.commonprefix([names[id(p)] for p in ps])
            got.append((prefix.split(".")[0] + ("." + prefix.split(".")[1] if prefix.startswith("body") else ""), lr))
        PG = {k: v for k, v in G.state_dict().items()}
        want = [(p.rstrip("."), lr) for p, lr in O.g_param_groups(PG, opt, scale_idx)]
        assert [(a, pytest.approx(b)) for a, b in got] == want


def test_compute_on_cpu_fails_loudly():
    from hp_vae_gan_amd import ops
    opt = opt_from(dict(nc_im=3, nfc=8, latent_dim=8, enc_blocks=2, ker_size=3, num_layer=5, padd_size=1, vae_levels=2, train_all=False))
    D = networks_3d.WDiscriminator3D(opt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D(torch.zeros(1, 3, 2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.MSE.apply(torch.zeros(4), torch.zeros(4))


def test_checkpoint_format_roundtrip(tmp_path):
    """Reference-format checkpoint files: keys, resume rule, D warm start (host logic only, CPU)."""
    from hp_vae_gan_amd import checkpoint as ck
    fx = load_golden("step3d_gan_s3.pt")
    opt = opt_from(fx["opt"], scale_idx=3, Noise_Amps=[1, 0.05, 0.06, 0.07])
    G = networks_3d.GeneratorHPVAEGAN(opt)
    for _ in range(3):
        G.init_next_stage()
    G.load_state_dict(fx["G_init"])
    D = networks_3d.WDiscriminator3D(opt)
    D.load_state_dict(fx["D_init"])

    class _Opt:
        def state_dict(self):
            return {"t": 0}

    class _Tr:
        netG, netD, optimizerG, optimizerD = G, D, _Opt(), _Opt()
    files = ck.stage_checkpoint(opt, _Tr)
    assert set(files) == {"Noise_Amps.pth", "netG.pth", "netD_3.pth"}
    assert set(files["netG.pth"]) == {"scale", "state_dict", "optimizer", "noise_amps"}
    assert set(files["netD_3.pth"]) == {"scale", "state_dict", "optimizer"}
    assert list(files["netG.pth"]["state_dict"].keys()) == list(fx["G_init"].keys())
    ck.save_stage(str(tmp_path), opt, _Tr)
    G2 = networks_3d.GeneratorHPVAEGAN(opt)
    scale, amps = ck.resume_generator(G2, str(tmp_path))
    assert scale == 3 and amps == [1, 0.05, 0.06, 0.07] and len(G2.body) == 3
    for k, v in G2.state_dict().items():
        assert torch.equal(v, fx["G_init"][k]), k
    D2 = ck.warm_start_discriminator(networks_3d.WDiscriminator3D(opt), str(tmp_path), 4)
    for k, v in D2.state_dict().items():
        assert torch.equal(v, fx["D_init"][k]), k


def test_no_memset_or_memcpy_nodes_in_the_kernels_sources():
    """hipMemsetAsync / hipMemcpyAsync become memset / memcpy NODES when an iteration is captured into a hipGraph, and on
    this runtime those nodes are not reliably ordered against the kernel nodes around them (replays
    trained NaNs).  The library therefore zero-fills and copies with kernels only."""
    import glob
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hp-vae-gan_amd", "csrc")
    for path in glob.glob(os.path.join(root, "*.hip")) + glob.glob(os.path.join(root, "*.h")):
        code = re.sub(r"//[^\n]*", "", open(path).read())           # comments may mention them
        assert "hipMemsetAsync" not in code and "hipMemcpyAsync" not in code and "hipMemset(" not in code, path


def test_flat_adam_state_dict_is_torch_adams(tmp_path):
    """optim.FlatAdam.state_dict() is torch.optim.Adam's layout: an Adam built over the same groups loads it, the moments
    land on the right parameters, the step count is the device counter's (the only one hipGraph replays advance), and the
    dict survives torch.save / weights_only load (what checkpoint.stage_checkpoint writes as 'optimizer')."""
    from hp_vae_gan_amd import optim as hp_optim
    from hp_vae_gan_amd import train as hp_train
    fx = load_golden("step3d_gan_s3_td2.pt")     # two trained blocks with different learning rates
    opt = opt_from(fx["opt"], scale_idx=3)
    G = networks_3d.GeneratorHPVAEGAN(opt)
    for _ in range(3):
        G.init_next_stage()
    arena = hp_optim.ParamArena(G)
    groups = [(list(ps), lr) for ps, lr in hp_train.generator_param_groups(opt, G)]
    adam = hp_optim.FlatAdam(arena, groups, betas=(0.5, 0.999))
    assert adam.state_dict()["state"] == {}          # nothing stepped yet: torch's Adam has no state either
    g = torch.Generator().manual_seed(3)
    for grp in adam.groups:
        grp["m"].copy_(torch.randn(grp["m"].shape, generator=g))
        grp["v"].copy_(torch.rand(grp["v"].shape, generator=g))
    adam.t_dev.fill_(7)                              # seven replayed steps: the host mirror adam.t never saw them
    sd = adam.state_dict()
    torch.save(sd, str(tmp_path / "opt.pt"))
    sd = torch.load(str(tmp_path / "opt.pt"), weights_only=True)
    ref = torch.optim.Adam([{"params": ps, "lr": lr} for ps, lr in groups], lr=opt.lr_g, betas=(0.5, 0.999))
    ref.load_state_dict(sd)
    assert [pg["lr"] for pg in ref.param_groups] == [lr for _, lr in groups] and len(groups) == 2 and groups[0][1] != groups[1][1]
    for (ps, _), grp in zip(groups, adam.groups):
        for p in ps:
            o, n = arena.range[id(p)]
            st = ref.state[p]
            assert float(st["step"]) == 7.0
            assert torch.equal(st["exp_avg"], grp["m"][o - grp["lo"]:o - grp["lo"] + n].view(p.shape))
            assert torch.equal(st["exp_avg_sq"], grp["v"][o - grp["lo"]:o - grp["lo"] + n].view(p.shape))


def test_narrow_conv_plan_keeps_every_load_inside_the_image():
    """conv_narrow2_kernel streams its input with 16-byte loads from column WINDOWS that must lie inside the image (nothing
    zeroes a halo column, nothing may be read before / after the tensor): host-side check of the planner's band table over
    every width the pyramids (and the padded baseline volumes) can produce."""
    import ctypes
    from hp_vae_gan_amd import lib as hplib
    lib = hplib.load()
    out = (ctypes.c_int * 55)()
    for Cout in (1, 3, 4):
        JB = 4 if 9 * Cout <= 32 else 2
        for W in list(range(4, 300)) + [512, 1000]:
            for H in (1, 3, 18, 91, 144):
                rc = lib.hpvg_conv_narrow_plan(2, 64, Cout, 5, H, W, 3, out)
                assert rc == 0, (Cout, W, H, rc)
                RS, Th, nth, nb, npos, G, pitch = list(out[:7])
                assert RS % 4 == 0 and 4 <= RS <= W and npos == (Th + 2) * RS and G * 32 * JB >= npos and pitch >= G * 32 * JB
                assert nth * Th >= H and (nth - 1) * Th < H
                assert 9 * Cout * pitch * 4 <= 76 * 1024
                nxt = 0
                for k in range(nb):
                    ws, ob, on = out[7 + 3 * k], out[8 + 3 * k], out[9 + 3 * k]
                    assert 0 <= ws and ws + RS <= W, (W, RS, k, ws)               # the window lies inside the image
                    assert ob == nxt and on >= 1                                  # outputs tile [0, W) without gaps
                    assert max(ob - 1, 0) >= ws and min(ob + on, W - 1) <= ws + RS - 1   # in-image neighbours are in the window
                    nxt = ob + on
                assert nxt == W
    assert lib.hpvg_conv_narrow_plan(2, 5, 3, 5, 9, 16, 3, out) != 0    # odd Cin: first-generation kernel
    assert lib.hpvg_conv_narrow_plan(2, 64, 3, 5, 9, 3, 3, out) != 0    # narrower than one 16-byte group


def test_graph_capture_refusal_restores_host_state(monkeypatch):
    """_capture_iteration on a stubbed device: when the captured graph holds a memset node the capture is refused
    with GraphCaptureRefused and everything the host advanced while RECORDING the iteration - the trainer's iteration count,
    BatchNorm's pending forward counts, the optimizers' step counts, the noise stream's call index - is back where it was, so
    a caller that catches the error trains on eagerly from a consistent state; the accepted capture keeps its replay deltas."""
    import contextlib
    import types
    import torch
    from hp_vae_gan_amd import train as T

    class _Stream:
        def wait_stream(self, other):
            pass

    class _Graph:
        def __init__(self, keep_graph=True):
            pass

        def instantiate(self):
            self.ok = True

    monkeypatch.setattr(torch.cuda, "Stream", _Stream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: _Stream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "CUDAGraph", _Graph)
    monkeypatch.setattr(torch.cuda, "graph", lambda g: contextlib.nullcontext())
    monkeypatch.setattr(T.ops, "pin_workspaces", lambda: None)
    census = {}
    monkeypatch.setattr(T, "graph_node_census", lambda g: dict(census))

    class BN(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.pending_batches = 7

    net = torch.nn.Sequential(BN(), BN())
    opt_g, opt_d = types.SimpleNamespace(t=11), types.SimpleNamespace(t=5)
    rng = types.SimpleNamespace(call=3)
    trainer = types.SimpleNamespace(iteration=4, optimizerG=opt_g, optimizerD=opt_d, opt=types.SimpleNamespace(device="cpu"), _graph=None)
    monkeypatch.setattr(T, "_host_state", lambda tr: {"opt": [(opt_g, opt_g.t), (opt_d, opt_d.t)], "rng": (rng, rng.call)})

    def run():   # what recording an iteration does to the host
        trainer.iteration += 1
        for m in net:
            m.pending_batches += 2
        opt_g.t += 1
        opt_d.t += 1
        rng.call += 9
        return {"loss": 1.0}

    census.update(kernel=40, memset=1)
    with pytest.raises(T.GraphCaptureRefused):
        T._capture_iteration(trainer, run, (net, None))
    # (the warm-up run on the side stream is a REAL iteration and counts: one run's worth; the recorded one is undone)
    assert trainer.iteration == 5 and [m.pending_batches for m in net] == [9, 9]
    assert (opt_g.t, opt_d.t, rng.call) == (12, 6, 12)
    assert trainer._graph is None and trainer._g_out is None

    census.clear()
    census.update(kernel=40)
    T._capture_iteration(trainer, run, (net, None))
    assert trainer.iteration == 6 and [m.pending_batches for m in net] == [11, 11]          # warm-up counted, recording undone
    assert trainer._graph is not None and trainer._g_out == {"loss": 1.0}
    assert [(m.pending_batches, d) for m, d in trainer._graph_bn] == [(11, 2), (11, 2)]    # what every replay adds


@pytest.mark.parametrize("kind", ["stage", "baseline"])
def test_alpha_source_seam(kind, monkeypatch):
    """The gradient penalty's alpha seam of both trainers on stub networks (no device): with alpha_source unset _step_eager
    takes the paths it always took - alpha None handed to calc_gradient_penalty (which draws torch.rand(1, 1) on the CPU
    generator), or, with _graph_alpha, torch.rand(1, device=...) per critic step; with it set, the source's own tensors reach
    calc_gradient_penalty, torch.rand is never called and the CPU generator does not move; an explicit alpha / alphas argument
    still wins."""
    import types
    from hp_vae_gan_amd import train as T

    class G(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

        def forward(self, x, amps, noise_init=None, mode="rand"):
            return x * self.w

        def forward_pair(self, rz, amps, noise_init):
            y = rz * self.w
            return y, y + 1, y, (y, y)

    class D(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

        def forward(self, x):
            return x * self.w

    seen = []

    def penalty(netD, real, fake, lam, device, alpha=None):
        seen.append(alpha)
        return (fake.detach() * netD.w).mean()

    monkeypatch.setattr(T, "calc_gradient_penalty", penalty)
    monkeypatch.setattr(T, "wgan_mean", lambda x, sign: sign * x.mean())
    monkeypatch.setattr(T, "mse_loss", lambda a, b: ((a - b) ** 2).mean())
    rand_calls = []
    real_rand = torch.rand
    monkeypatch.setattr(torch, "rand", lambda *a, **k: rand_calls.append((a, k)) or real_rand(*a, **k))

    def arena():
        return types.SimpleNamespace(zero_grad=lambda: None, clip_grad_norm_=lambda *a: None, grad=None)

    def adam():
        return types.SimpleNamespace(step=lambda: None)

    Dsteps = 2 if kind == "baseline" else 1
    opt = types.SimpleNamespace(Noise_Amps=[1], lambda_grad=0.1, device="cpu", Dsteps=Dsteps, Gsteps=1, disc_loss_weight=1.0,
                                rec_weight=10.0, alpha=10.0, grad_clip=5.0, Z_init=torch.zeros(1, 1, 2, 2, 2), scale_idx=1)
    cls = T.StageTrainer if kind == "stage" else T.BaselineStageTrainer
    tr = cls.__new__(cls)
    tr.__dict__.update(opt=opt, netG=G(), netD=D(), is_gan=True, arenaG=arena(), arenaD=arena(), optimizerG=adam(), optimizerD=adam(),
                       after_d_step=None, loss_log=None, iteration=1, clip_info=torch.zeros(2), last={},
                       alpha_source=getattr(opt, "alpha_source", None))
    real = torch.full((1, 1, 2, 2, 2), 0.5)
    noise_init = torch.zeros(1, 1, 2, 2, 2)

    def step(**kw):
        del seen[:], rand_calls[:]
        before = torch.get_rng_state()
        if kind == "stage":
            tr._step_eager(real, real, noise_init, **kw)
        else:
            tr._step_eager(real, noise_init, **kw)
        assert len(seen) == Dsteps
        return torch.equal(before, torch.get_rng_state())

    # unset: today's paths
    assert tr.alpha_source is None
    assert step() and seen == [None] * Dsteps and not rand_calls          # (calc_gradient_penalty itself draws on the CPU generator)
    tr._graph_alpha = True
    assert not step() and len(rand_calls) == Dsteps                       # torch.rand(1, device=real.device): one per critic step
    assert all(a == (1,) and k == {"device": real.device} for a, k in rand_calls)
    assert all(torch.is_tensor(a) and a.shape == (1,) for a in seen)
    # set: the source's tensors, nothing drawn - in eager mode and in the mode enable_graph switches on
    buf = torch.tensor([0.25, 0.75])
    views = [buf[j:j + 1] for j in range(Dsteps)]
    asked = []
    tr.alpha_source = lambda n, device: asked.append((n, device)) or views
    for graph_alpha in (False, True):
        tr._graph_alpha = graph_alpha
        del asked[:]
        assert step() and not rand_calls
        assert asked == [(Dsteps, real.device)]
        assert len(seen) == Dsteps and all(a is v for a, v in zip(seen, views))
    # an explicit argument wins over the source
    mine = [torch.tensor([0.5]) for _ in range(Dsteps)]
    del asked[:]
    assert step(**({"alpha": mine[0]} if kind == "stage" else {"alphas": mine})) and not asked and not rand_calls
    assert all(a is m for a, m in zip(seen, mine))


def test_two_axis_conv_is_bounded_by_its_zero_plane_and_offsets():
    """conv_wino2r_kernel stages a time plane outside the clip from a device plane of zeros (2^18 floats) and addresses its
    epilogue with 32-bit offsets: the size rule (host only) must hand larger planes / volumes to the one-axis kernel (kind 1)
    and keep the pyramid's big shapes on the two-axis kernel (kind 2)."""
    lib = hplib.load()
    kind = lib.hpvg_conv_fwd_kernel_kind
    # the size rule by size: the library's default mode (1), whatever an earlier test of this process left configured
    prev = lib.hpvg_conv_wino_config(-1, -1)
    assert lib.hpvg_conv_wino_config(1, -1) == 1
    try:
        _two_axis_bounds(kind)
    finally:
        lib.hpvg_conv_wino_config(prev, -1)


def _two_axis_bounds(kind):
    assert kind(2, 64, 64, 13, 144, 256, 3) == 2          # stage 9 of the BASELINE video config
    assert kind(2, 64, 64, 7, 114, 204, 3) == 2           # stage 8
    assert kind(2, 64, 64, 5, 1000, 256, 3) == 2          # a plane of 256 000 floats: below the zero plane's 2^18
    assert kind(2, 64, 64, 5, 1024, 256, 3) != 2          # 2^18 floats + the 4 the check keeps free: too large
    assert kind(2, 64, 64, 5, 1100, 256, 3) != 2
    assert kind(2, 64, 64, 5, 512, 512, 3) != 2           # (a tile's staged span must fit 1024 floats: W <= 256 for half-row tiles)
    assert kind(2, 64, 64, 13, 144, 256, 1) != 2          # the 2-D convs never run it
