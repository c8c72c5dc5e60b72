"""Host check (no GPU) of the forward / backward-data convolution decisions of csrc/conv_mfma.hip: which kernel family runs a
shape, the scratch it asks for, whether its weight pack carries the two-axis Winograd section and how large that pack is, and
the three tile plans, under every run-time mode and every environment knob that moves them, against
tests/golden/conv_fwd_decisions.json.

The table holds this project's own answers, recorded before the host path was reorganised
(`python tests/test_conv_fwd_decisions_host.py --record`).  It is a safety net for refactors, not a specification: a change of
a size rule or a planner changes it on purpose and records it again."""
import ctypes
import json
import os
import struct
import subprocess
import sys
import zlib

import conv_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_fwd_decisions.json")
MODES = (0, 1, 2, 3, 4, 5, 6)
MIN_POSITIONS = (0, 10 ** 9)
# one child process each, no mode set: the knobs are read once per process
CHILD_ENVS = ("HPVG_WINO=0", "HPVG_WINO_MIN=0", "HPVG_WINO_STG=1", "HPVG_WINO_STG=2", "HPVG_WINO2D=0", "HPVG_WINO2R=0",
              "HPVG_PLAN_NB=1", "HPVG_PLAN_MB=1", "HPVG_PLAN_NTW=2")
KNOBS = ("HPVG_WINO", "HPVG_WINO_MIN", "HPVG_WINO_STG", "HPVG_WINO2D", "HPVG_WINO2R", "HPVG_WINO_STAGGER", "HPVG_CONV_SK",
         "HPVG_NARROW2", "HPVG_PLAN_NB", "HPVG_PLAN_MB", "HPVG_PLAN_NTW")
COLUMNS = ["B", "Cin", "Cout", "T", "H", "W", "KT", "kernel_kind", "ws_bytes", "wants_wino2d", "wpack_floats_for", "plans_crc32"]
ABOUT = ("Every distinct row once; a walk (a run-time mode, a Winograd threshold, or an environment knob in a fresh process) "
         "lists its rows by index, in the order of cases().  Answers of this project's own forward-convolution host queries "
         "(hpvg_conv_fwd_kernel_kind, _fwd_ws_bytes, _wants_wino2d, _wpack_floats_for and a CRC-32 over the return codes and "
         "out[] arrays of _fwd_plan, _wino_plan and _narrow_plan), recorded by tests/test_conv_fwd_decisions_host.py --record.  "
         "Nothing here comes from the reference implementation.")
PLANS = (("hpvg_conv_fwd_plan", 10), ("hpvg_conv_wino_plan", 10), ("hpvg_conv_narrow_plan", 7 + 3 * 16))


def cases():
    """(B, Cin, Cout, T, H, W, KT) of every checked launch, each once: the pyramids' launches forward and backward-data (Cin
    and Cout swapped), the shapes of the forward GPU tests of test_hip_ops.py, those of the two host tests of the two-axis
    size rule and the narrow plan, and KT = 2.  Thinned to keep the table near 100 KB: the wide layers, whose kernel the
    batch size decides, at every batch size of the video and image pyramids; the heads and tails, and the video8 pyramid, at
    B = 2; the narrow plan at the widths and heights where its band table changes form."""
    import test_hip_ops
    out = []
    video8 = list(R.KINDS)[10:17]
    for sp in R.KINDS:
        for Ci, Co in R.KIND_LAYERS:
            for B in R.BATCHES if min(Ci, Co) > 4 and sp not in video8 else (2,):
                out.append((B, Ci, Co) + R.kernel_view(sp))
                out.append((B, Co, Ci) + R.kernel_view(sp))
    for fn in (test_hip_ops.test_conv_winograd_kernel_against_direct_kernel_and_oracle,
               test_hip_ops.test_conv_winograd_two_axis_kernel_against_direct_kernel_and_oracle):
        (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
        for B, Cin, Cout, sp in mark.args[1]:
            out.append((B, Cin, Cout) + R.kernel_view(sp))
            out.append((B, Cout, Cin) + R.kernel_view(sp))
    for B, Cin, Cout, sp in test_hip_ops.CONV_CASES:
        out.append((B, Cin, Cout) + R.kernel_view(sp))
        out.append((B, Cout, Cin) + R.kernel_view(sp))
    # test_two_axis_conv_is_bounded_by_its_zero_plane_and_offsets
    for T, H, W, KT in ((13, 144, 256, 3), (7, 114, 204, 3), (5, 1000, 256, 3), (5, 1024, 256, 3), (5, 1100, 256, 3),
                        (5, 512, 512, 3), (13, 144, 256, 1)):
        out.append((2, 64, 64, T, H, W, KT))
    # test_narrow_conv_plan_keeps_every_load_inside_the_image
    for Cout in (1, 3, 4):
        for W in (4, 7, 33, 257, 1000):
            for H in (1, 144):
                out.append((2, 64, Cout, 5, H, W, 3))
    out += [(2, 5, 3, 5, 9, 16, 3), (2, 64, 3, 5, 9, 3, 3)]
    out += [(1, 1, 1, 1, 1, 1, 2), (1, 64, 64, 2, 8, 8, 2), (2, 64, 3, 2, 8, 8, 2)]
    return list(dict.fromkeys(out))


def rows(lib):
    """One row of COLUMNS per case, under the mode and environment in force."""
    res = []
    for c in cases():
        B, Cin, Cout, T, H, W, KT = c
        blob = b""
        for name, n in PLANS:
            out = (ctypes.c_int * n)(*([-7] * n))      # (what a query leaves unwritten stays -7)
            rc = getattr(lib, name)(*c, out)
            blob += struct.pack("<%di" % (n + 1), rc, *out)
        res.append(list(c) + [lib.hpvg_conv_fwd_kernel_kind(*c), lib.hpvg_conv_fwd_ws_bytes(*c), lib.hpvg_conv_wants_wino2d(*c),
                              lib.hpvg_conv_wpack_floats_for(Cin, Cout, KT, B, T, H, W), zlib.crc32(blob)])
    return res


def _lib():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


def walk_modes(lib):
    """[{"mode=N": rows}, the same of a second pass, {"min_positions=N": rows}]: modes 0..6 in order (3 and 4 force a staging
    form of the one-axis kernel, so the plans of a shape change between them), again from warm memos, then mode 1 with the
    Winograd threshold at both ends.  The threshold has no way back to its per-kernel-size default, so that walk comes last
    and this runs in a process of its own."""
    prev = lib.hpvg_conv_wino_config(-1, -1)
    passes = []
    try:
        for _ in range(2):
            got = {}
            for mode in MODES:
                assert lib.hpvg_conv_wino_config(mode, -1) == mode
                got["mode=%d" % mode] = rows(lib)
            passes.append(got)
        got = {}
        for n in MIN_POSITIONS:
            assert lib.hpvg_conv_wino_config(1, n) == 1
            got["min_positions=%d" % n] = rows(lib)
        passes.append(got)
    finally:
        lib.hpvg_conv_wino_config(prev, -1)
    return passes


def walk_children(envs):
    """{env: what a fresh process prints with it set}, all started at once and with no other knob of KNOBS set: walk_modes's
    passes for "" (the knobs are read once per process, and a test before this one may have switched modes), else the rows
    of the process as it starts."""
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    procs = [(e, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child-env" if e else "--child-modes"],
                                  env=dict(base, **dict([e.split("=")] if e else [])), stdout=subprocess.PIPE)) for e in envs]
    got = {}
    for e, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, "child %r: exit status %d" % (e, p.returncode)
        got[e] = json.loads(out)
    return got


def _child(modes):
    lib = _lib()
    json.dump(walk_modes(lib) if modes else rows(lib), sys.stdout)


def _differences(tag, got, want):
    if len(got) != len(want):
        return ["%s: %d rows, table %d" % (tag, len(got), len(want))]
    return ["%s: %s\n%*s table %s" % (tag, dict(zip(COLUMNS, g)), len(tag), "", dict(zip(COLUMNS, w)))
            for g, w in zip(got, want) if g != w]


def _table():
    """{walk: rows} of the committed table, which stores every distinct row once and each walk as indices into them."""
    with open(GOLDEN) as f:
        t = json.load(f)
    return {tag: [t["rows"][i] for i in idx] for tag, idx in t["walks"].items()}


def _wrapped(items, indent):
    """The JSON texts `items`, comma-separated, on lines of up to 128 characters."""
    lines, line = [], indent
    for k, it in enumerate(items):
        it += "," if k + 1 < len(items) else ""
        if len(line) + len(it) > 128 and line != indent:
            lines.append(line)
            line = indent
        line += it
    return "\n".join(lines + [line])


def _report(bad):
    if bad:
        print("\n".join(bad))
    assert not bad, "%d rows differ from tests/golden/conv_fwd_decisions.json (printed in full above)" % len(bad)


def test_decisions_under_every_mode_cold_and_warm_and_both_thresholds():
    want = _table()
    first, second, thresholds = walk_children([""])[""]
    bad = []
    for tag in first:
        bad += _differences(tag, first[tag], want[tag])
        bad += _differences(tag + " (second pass)", second[tag], want[tag])
    for tag in thresholds:
        bad += _differences(tag, thresholds[tag], want[tag])
    _report(bad)
    kinds = set(r[7] for rs in first.values() for r in rs if r[6] != 2)
    assert kinds == {0, 1, 2, 3}, kinds


def test_decisions_under_every_environment_knob():
    want = _table()
    got = walk_children(CHILD_ENVS)
    bad = []
    for tag in CHILD_ENVS:
        bad += _differences(tag, got[tag], want[tag])
    _report(bad)


def _record():
    got = walk_children(("",) + CHILD_ENVS)
    first, second, thresholds = got.pop("")
    assert first == second, "the second pass (warm memos) differs from the first"
    walks = dict(first, **thresholds, **got)
    index = {}
    for rs in walks.values():
        for r in rs:
            index.setdefault(tuple(r), len(index))
    with open(GOLDEN, "w") as f:
        f.write('{"about": %s,\n "columns": %s,\n "rows": [\n' % (json.dumps(ABOUT), json.dumps(COLUMNS)))
        f.write(_wrapped([json.dumps(r, separators=(",", ":")) for r in index], "  "))
        f.write('],\n "walks": {\n')
        f.write(",\n".join('  %s: [\n%s]' % (json.dumps(tag), _wrapped([str(index[tuple(r)]) for r in rs], "   "))
                           for tag, rs in walks.items()))
        f.write("\n }}\n")
    print("%s: %d walks, %d rows, %d distinct" % (GOLDEN, len(walks), sum(len(rs) for rs in walks.values()), len(index)))


if __name__ == "__main__":
    if "--child-modes" in sys.argv or "--child-env" in sys.argv:
        _child("--child-modes" in sys.argv)
    elif "--record" in sys.argv:
        _record()
    else:
        sys.exit("usage: %s --record" % sys.argv[0])
