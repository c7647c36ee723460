"""The inventory of the shipped A/B switches (no GPU needed): every slak_env_flag("NAME", default) call site of slak_amd/csrc/ has an entry in
tests/ab_switches.py's SWITCHES -- with the call site's default and the value that flips it -- and every entry has a call site, so a switch added
later without a case in tests/test_ab_switches_gpu.py fails here.  What the table pins about a DEFAULT process (the block-tail families, the MLP rungs)
is host code and is held here too."""
import glob
import json
import os
import re
import subprocess
import sys

import ab_switches as ab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call_sites():
    """{name: {defaults at its call sites}}"""
    sites = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "slak_amd", "csrc", "*"))):
        for name, default in re.findall(r'slak_env_flag\(\s*"(\w+)"\s*,\s*(true|false)\s*\)', open(path).read()):
            sites.setdefault(name, set()).add(default == "true")
    return sites


def test_every_switch_has_a_case_and_every_case_a_switch():
    sites = _call_sites()
    assert len(sites) >= 26, sorted(sites)                  # (the pattern still finds the call sites)
    assert set(sites) == set(ab.SWITCHES), sorted(set(sites) ^ set(ab.SWITCHES))
    for name, sw in ab.SWITCHES.items():
        assert sites[name] == {sw["default"]}, (name, sites[name])
        assert sw["flip"] == ("0" if sw["default"] else "1"), name
        assert bool(sw["cases"]) != bool(sw["covered_by"]), name     # a case, or the test that flips the switch through another door
    assert [n for n, sw in ab.SWITCHES.items() if sw["covered_by"]] == ["SLAK_FP32_MFMA"]
    assert sorted(n for n, sw in ab.SWITCHES.items() if sw["no_observable"]) == ["SLAK_LN_CF_REG", "SLAK_RT_WIDE", "SLAK_SMALL_QUAD", "SLAK_TRI_ROWS_SD"]


def test_the_pinned_switch_tables_cover_every_conv_switch_and_its_cases():
    pinned = json.load(open(ab.PINNED))
    base = json.load(open(os.path.join(ROOT, "tests", "golden", "dispatch_table_small.json")))
    assert set(pinned) == {n for n in ab.CASE_SWITCHES if ab.SWITCHES[n]["group"] in ("conv", "tail")}
    for name in ab.CONV_SWITCHES:
        sw, diff = ab.SWITCHES[name], pinned[name]
        assert len(sw["cases"]) <= (4 if sw["no_observable"] else 3), name
        assert all(base.get(k) != v for k, v in diff.items()), name          # only the keys that differ from the default table
        if sw["no_observable"]:
            assert not diff, name
            continue
        assert diff, name + " changes no launch of the table's shapes"
        for case in sw["cases"]:                             # every case is a shape on which the switch changes a launch ...
            assert any(k.startswith(ab.case_keys(case)) for k in diff), (name, case)
        # ... and every kind of launch it changes anywhere (the op and, for the per-branch entry points, the filter's orientation) is met on one of them
        def kind(k):
            parts = k.split("/")
            if parts[1] in ("tri", "pair"):
                return "/".join(parts[1:])
            kh, kw = (int(v) for v in (parts[1] if "x" in parts[1] and parts[1][0].isdigit() else parts[0].split("_")[-1]).split("x"))
            return ("Kx5" if kh > kw else "5xK" if kw > kh else "5x5") + "/" + parts[-1]
        met = {kind(k) for k in diff if any(k.startswith(ab.case_keys(c)) for c in sw["cases"])}
        assert {kind(k) for k in diff} == met, (name, sorted({kind(k) for k in diff} - met))


def test_a_default_process_answers_what_the_table_calls_the_default():
    lib = ab.load("slak_amd/_lib.py", "_slak_lib_only")
    L = lib.lib()
    assert not [n for n in ab.SWITCHES if n in os.environ]
    pinned = json.load(open(ab.PINNED))
    for name in ab.CASE_SWITCHES:
        sw = ab.SWITCHES[name]
        if sw["group"] == "tail":
            assert pinned[name] == {ab.tail_key(c): ab.tail_families(L, lib, c) for c in sw["cases"]}, name
        for case, (default, flipped) in sw.get("stats_rows", {}).items():
            assert L.slak_dwconv2d_tri_stats_rows(lib.SLAK_BF16, *case) == default != flipped, (name, case)
        if sw["group"] == "pointwise":
            for case in sw["cases"]:
                rungs = ab.mlp_rungs(L, lib, case["M"], case["C"])
                assert {k: rungs[k] for k in case["default"]} == case["default"], (name, case, rungs)
                assert set(case["expect"]) == set(case["default"]) and all(case["expect"][k] != case["default"][k] for k in case["expect"]), (name, case)


def test_size_queries_answer_for_the_switches_their_launches_honour():
    """The pair, three-branch and one-launch-backward weight gradients finish through the arrival counters and the pair launch is the LDS-DMA kernels' alone:
    with SLAK_WGRAD_REDUCE=1 resp. SLAK_MFMA_DMA=0 those launches refuse, so their size / support queries must answer 0 in such a process (they said yes before,
    and the launch then refused what the query had promised).  Host code: one short child process per switch."""
    code = ("import importlib.util, json, sys; spec = importlib.util.spec_from_file_location('_l', sys.argv[1]); lib = importlib.util.module_from_spec(spec); "
            "spec.loader.exec_module(lib); L = lib.lib(); B = lib.SLAK_BF16; "
            "print(json.dumps([L.slak_dwconv2d_pair_filter_workspace_bytes(B, 3, 2, 56, 56, 51), L.slak_dwconv2d_pair_filter_workspace_bytes(B, 9, 2, 28, 28, 49), "
            "L.slak_dwconv2d_tri_filter_workspace_bytes(B, 3, 2, 56, 56, 51), L.slak_dwconv2d_tri_filter_workspace_bytes(B, 9, 2, 28, 28, 49), "
            "L.slak_dwconv2d_tri_filter_workspace_bytes(B, 5, 7, 14, 14, 47), L.slak_dwconv2d_tri_backward_supported(B, 5, 7, 14, 14, 47)]))")

    def ask(**env):
        r = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "slak_amd", "_lib.py")], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.splitlines()[-1])
    assert all(v > 0 for v in ask())
    assert ask(SLAK_WGRAD_REDUCE="1") == [0, 0, 0, 0, 0, 0]
    dma_off = ask(SLAK_MFMA_DMA="0")
    assert dma_off[:2] == [0, 0] and all(v > 0 for v in dma_off[2:])     # the three-branch kernels do not go through the DMA switch
