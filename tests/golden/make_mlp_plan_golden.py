"""Writes tests/golden/mlp_plan.json: which launch runs each step of a block's pointwise MLP, for every point of GRID.

    python tests/golden/make_mlp_plan_golden.py [--lib PATH/libslak_hip.so] [--out PATH.json]

The independent restatement of the ladder that slak_mlp_plan (include/slak_hip.h) answers: evaluated here from the primitive slak_linear_*_supported /
*_workspace_bytes queries ONLY -- this script never calls slak_mlp_plan, so it runs unchanged on a library from before that query existed (the
recording was made on such a library and on the first one with the query: byte-identical files).  Host code only, no GPU needed; without a device the
CU count the queries use falls back to the MI355X's 256 (tests/test_mlp_plan_cpu.py skips on a device with another count).

Two of the rungs exist at the default switches on no shape: pwconv1 through slak_linear_nt(gelu) is shadowed by slak_linear_mlp_fwd and
slak_linear_nt_gelu_bwd by its _dt form wherever they apply.  The library's own A/B switches SLAK_LINEAR_MLP_FWD=0 and SLAK_LINEAR_GELU_BWD_DT=0
uncover them; each is recorded over the whole grid by a child process (the library reads a switch once per process)."""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "..", "..", "slak_amd", "lib", "libslak_hip.so")
LIBRARY, NT, GEMM, FUSED, FUSED_DT, KERNEL = 0, 1, 2, 3, 4, 5         # SLAK_MLP_* of include/slak_hip.h
SKINNY, GEMMS, WGRAD, ALL = 1, 2, 4, 7                                # SLAK_MLP_ALLOW_*
EPI_GELU, EPI_DGELU = 1, 2
FIELDS = ["pw1", "pw2", "dy1", "dt", "dw1", "dw2", "splits", "ws_dy1", "ws_dw1", "ws_dw2"]
MS = [1, 31, 32, 98, 128, 6272, 12544, 25088, 401408]
CPS = [64, 96, 104, 128, 192, 256, 384, 512, 768, 1024]
ALLOWS = [ALL, ALL & ~SKINNY, ALL & ~GEMMS, ALL & ~WGRAD]
GRID = [(M, 4 * Cp, Cp, allow) for M in MS for Cp in CPS for allow in ALLOWS]
SWITCHES = ["SLAK_LINEAR_MLP_FWD", "SLAK_LINEAR_GELU_BWD_DT"]         # each recorded at "0" in a process of its own
SPLITK_ROWS = 6272


def load(path):
    L = ctypes.CDLL(path)
    for name in ("slak_linear_nt_gelu_bwd_workspace_bytes", "slak_linear_gemm_workspace_bytes", "slak_linear_wgrad_workspace_bytes", "slak_gelu_bwd_workspace_bytes"):
        getattr(L, name).restype = ctypes.c_size_t
    return L


def ladder(L, M, C4, Cp, allow):
    """One row of FIELDS: the first rung of every step, in the order of the table, that the library supports and `allow` admits."""
    sk, ge, wg = bool(allow & SKINNY), bool(allow & GEMMS), bool(allow & WGRAD)
    if sk and L.slak_linear_mlp_fwd_supported(M, Cp, C4):
        pw1 = FUSED
    elif sk and L.slak_linear_nt_supported(M, C4, Cp, 1):
        pw1 = NT
    elif ge and L.slak_linear_gemm_supported(M, C4, Cp, EPI_GELU):
        pw1 = GEMM
    else:
        pw1 = LIBRARY
    pw2 = NT if sk and L.slak_linear_nt_supported(M, Cp, C4, 0) else LIBRARY
    if sk and L.slak_linear_nt_gelu_bwd_supported(M, C4, Cp):
        dy1 = FUSED_DT if L.slak_linear_nt_gelu_bwd_dt_supported(M, C4, Cp) else FUSED
        ws_dy1 = L.slak_linear_nt_gelu_bwd_workspace_bytes(M, C4, Cp)
    elif ge and L.slak_linear_gemm_supported(M, C4, Cp, EPI_DGELU):
        dy1 = GEMM
        ws_dy1 = L.slak_linear_gemm_workspace_bytes(M, C4, Cp, EPI_DGELU)
    else:
        dy1 = NT if sk and L.slak_linear_nt_supported(M, C4, Cp, 0) else LIBRARY
        ws_dy1 = L.slak_gelu_bwd_workspace_bytes(M, C4)
    dt = NT if sk and L.slak_linear_nt_supported(M, Cp, C4, 0) else LIBRARY
    dw1 = KERNEL if wg and L.slak_linear_wgrad_supported(M, C4, Cp) else LIBRARY
    dw2 = KERNEL if wg and L.slak_linear_wgrad_supported(M, Cp, C4) else LIBRARY
    S = max(1, M // SPLITK_ROWS)
    while S > 1 and M % S:
        S -= 1
    ws_dw1 = L.slak_linear_wgrad_workspace_bytes(M, C4, Cp) if dw1 == KERNEL else 0
    ws_dw2 = L.slak_linear_wgrad_workspace_bytes(M, Cp, C4) if dw2 == KERNEL else 0
    return [int(v) for v in (pw1, pw2, dy1, dt, dw1, dw2, S, ws_dy1, ws_dw1, ws_dw2)]


def rows(lib_path):
    L = load(lib_path)
    return [ladder(L, *point) for point in GRID]


def in_child(script, switch, *args):
    """What `script --rows ARGS` prints (JSON) in a fresh process with `switch`=0."""
    env = dict(os.environ)
    env[switch] = "0"
    return json.loads(subprocess.run([sys.executable, script, "--rows"] + list(args), env=env, check=True, stdout=subprocess.PIPE).stdout)


def dumps(doc):
    """One grid point per line."""
    head = {k: v for k, v in doc.items() if k != "rows"}
    body = ",\n".join('  "%s": [\n%s\n  ]' % (name, ",\n".join("    " + json.dumps(r) for r in rs)) for name, rs in doc["rows"].items())
    return json.dumps(head)[:-1] + ', "rows": {\n' + body + "\n}}\n"


if __name__ == "__main__":
    arg = lambda flag, default: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default
    lib_path = os.path.abspath(arg("--lib", DEFAULT_LIB))
    if "--rows" in sys.argv:
        print(json.dumps(rows(lib_path)))
    else:
        doc = {"fields": FIELDS, "grid": "(M, C4 = 4 Cp, Cp, allow) for M in M for Cp in Cp for allow in allow", "M": MS, "Cp": CPS, "allow": ALLOWS,
               "rows": {"default": rows(lib_path)}}
        for name in SWITCHES:
            doc["rows"][name + "=0"] = in_child(os.path.abspath(__file__), name, "--lib", lib_path)
        with open(arg("--out", os.path.join(HERE, "mlp_plan.json")), "w") as f:
            f.write(dumps(doc))
