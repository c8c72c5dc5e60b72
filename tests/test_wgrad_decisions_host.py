"""Host check (no GPU) of the weight-gradient decisions of csrc/conv_wgrad.hip: which kernel family runs a shape, whether
the launch fuses the bias gradient, the scratch it asks for and the three tile plans, under every run-time mode and every
environment knob that moves them, against tests/golden/wgrad_decisions.json.

The table holds this project's own answers, recorded before the host path was reorganised
(`python tests/test_wgrad_decisions_host.py --record`).  It is a safety net for refactors, not a specification: a change of
a size rule or a planner changes it on purpose and records it again."""
import ctypes
import json
import os
import struct
import subprocess
import sys
import zlib

import conv_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_decisions.json")
MODES = (0, 1, 2, 3, 4, 5, 6)
# one child process each, no mode set: the knobs are read once per process
CHILD_ENVS = ("HPVG_WGRAD3=0", "HPVG_WGRAD3=2", "HPVG_WGRAD_WINO=0", "HPVG_WGRADW2=1", "HPVG_WGRADW2=2", "HPVG_WGRADW_G16=0",
              "HPVG_WGRAD_BALANCE=0", "HPVG_WGRADW2_MIN_TILES=8")
KNOBS = ("HPVG_WGRAD_WINO", "HPVG_WGRADW2", "HPVG_WGRADW2_MIN_TILES", "HPVG_WGRADW_G16", "HPVG_WGRADW_W8", "HPVG_WGRADW_WCH",
         "HPVG_WGRAD3", "HPVG_WGRAD_NARROW2", "HPVG_WGRAD_BALANCE", "HPVG_WG2_ORDER", "HPVG_WG16_FORCE", "HPVG_WG2_FORCE")
COLUMNS = ["B", "Cin", "Cout", "T", "H", "W", "KT", "kernel_kind", "fuses_bias", "ws_bytes", "plans_crc32"]
ABOUT = ("Every distinct row once; a walk (a run-time mode, or an environment knob in a fresh process) lists its rows by "
         "index, in the order of cases().  Answers of this project's own weight-gradient host queries (hpvg_conv_bwd_weight_kernel_kind, _fuses_bias, "
         "_ws_bytes and a CRC-32 over the return codes and out[] arrays of _plan, _wino_plan and _wino2_plan), recorded by "
         "tests/test_wgrad_decisions_host.py --record.  Nothing here comes from the reference implementation.")


def cases():
    """(B, Cin, Cout, T, H, W, KT) of every checked launch: the pyramids' launches, the shapes of the Winograd weight-gradient
    GPU test without its two largest, and a few degenerate ones."""
    import test_hip_ops
    out = []
    for sp in R.KINDS:
        for layer in R.KIND_LAYERS:
            for B in R.BATCHES:
                out.append((B,) + tuple(layer) + R.kernel_view(sp))
    fn = test_hip_ops.test_conv_weight_gradient_winograd_kernel_against_direct_kernels_and_oracle
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]

    def size(c):
        n = c[0] * c[1] * c[2]
        for v in c[3]:
            n *= v
        return n
    for B, Cin, Cout, sp in sorted(mark.args[1], key=size)[:-2]:
        out.append((B, Cin, Cout) + R.kernel_view(sp))
    for Cin, Cout, sp in ((3, 64, (2, 3, 3)), (64, 1, (1, 2, 3)), (4, 4, (2, 5, 5)), (64, 3, (5, 9, 3))):
        out.append((1, Cin, Cout) + R.kernel_view(sp))
    return out


def rows(lib):
    """One row of COLUMNS per case, under the mode and environment in force."""
    res = []
    for c in cases():
        blob = b""
        for name, n in (("hpvg_conv_bwd_weight_plan", 10), ("hpvg_conv_bwd_weight_wino_plan", 10),
                        ("hpvg_conv_bwd_weight_wino2_plan", 11)):
            out = (ctypes.c_int * n)(*([-7] * n))      # (what a query leaves unwritten stays -7)
            rc = getattr(lib, name)(*c, out)
            blob += struct.pack("<%di" % (n + 1), rc, *out)
        res.append(list(c) + [lib.hpvg_conv_bwd_weight_kernel_kind(*c), lib.hpvg_conv_bwd_weight_fuses_bias(*c),
                              lib.hpvg_conv_bwd_weight_ws_bytes(*c), zlib.crc32(blob)])
    return res


def _lib():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


def walk_modes(lib):
    """[{"mode=N": rows}, the same of a second pass]: modes 0..6 in order (3 and the step past it toggle the 16-byte form and
    drop the one-axis plans), then again from warm memos."""
    prev = lib.hpvg_conv_bwd_weight_wino_config(-1)     # (also settles the defaults)
    passes = []
    try:
        for _ in range(2):
            got = {}
            for mode in MODES:
                lib.hpvg_conv_bwd_weight_wino_config(mode)
                got["mode=%d" % mode] = rows(lib)
            passes.append(got)
    finally:
        lib.hpvg_conv_bwd_weight_wino_config(prev)
    return passes


def walk_children(envs):
    """{env: what a fresh process prints with it set}, all started at once and with no other knob of KNOBS set: walk_modes's
    two passes for "" (the knobs are read once per process, and a test before this one may have switched modes), else the
    rows after the -1 query alone."""
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
    lib.hpvg_conv_bwd_weight_wino_config(-1)
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


def test_decisions_under_every_mode_cold_and_warm():
    want = _table()
    first, second = walk_children([""])[""]
    bad = []
    for tag in first:
        bad += _differences(tag, first[tag], want[tag])
        bad += _differences(tag + " (second pass)", second[tag], want[tag])
    if bad:
        print("\n".join(bad))
    assert not bad, "%d rows differ from tests/golden/wgrad_decisions.json (printed in full above)" % len(bad)
    kinds = set(r[7] for rs in first.values() for r in rs)
    assert kinds == {0, 1, 2, 3, 4}, kinds


def test_decisions_under_every_environment_knob():
    want = _table()
    got = walk_children(CHILD_ENVS)
    bad = []
    for tag in CHILD_ENVS:
        bad += _differences(tag, got[tag], want[tag])
    if bad:
        print("\n".join(bad))
    assert not bad, "%d rows differ from tests/golden/wgrad_decisions.json (printed in full above)" % len(bad)


def _record():
    got = walk_children(("",) + CHILD_ENVS)
    first, second = got.pop("")
    assert first == second, "the second pass (warm memos) differs from the first"
    walks = dict(first, **got)
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
    print("%s: %d walks, %d rows" % (GOLDEN, len(walks), sum(len(rs) for rs in walks.values())))


if __name__ == "__main__":
    if "--child-modes" in sys.argv or "--child-env" in sys.argv:
        _child("--child-modes" in sys.argv)
    elif "--record" in sys.argv:
        _record()
    else:
        sys.exit("usage: %s --record" % sys.argv[0])
