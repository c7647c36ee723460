"""Every shipped A/B switch (tests/ab_switches.py's SWITCHES) flipped in a process of its own -- a switch is read once per process -- on the
MI355X: the child (python tests/ab_switches.py NAME) proves that the flag changed what runs, runs the affected entry points against the C oracle /
the fp64 references with the bounds of the default-path tests, and records every launch that refused after its query had said yes.  The older
kernels behind the switches are what a bisect or an A/B run trusts; the parity tests' shapes have long gone to their replacements.

One child at a time.  A child that ends by a signal, by an abort or at its time limit fails its case and latches: no later case starts a process."""
import json
import os
import subprocess
import sys

import pytest

import ab_switches as ab

pytestmark = pytest.mark.gpu

# Child wall times measured on an MI355X over three runs, interpreter start and GPU initialisation included: 2.2 .. 3.0 s for a conv switch (the small dispatch
# table included), 2.9 .. 3.5 s for a block-tail switch, 3.0 .. 4.1 s for a pointwise one.  Four times the slowest (16.5 s), rounded up to 30 s: the margin is for
# a busy shared host
CHILD_TIMEOUT_S = 30
_fault = []                                                  # the latch: [what ended badly]


def _run_child(name):
    sw = ab.SWITCHES[name]
    if _fault:
        pytest.fail("not started: %s" % _fault[0], pytrace=False)
    cmd = [sys.executable, os.path.join(ab.TESTS, "ab_switches.py"), name]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, **{name: sw["flip"]}), capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        _fault.append("the child of %s ran into its time limit (%d s)" % (name, CHILD_TIMEOUT_S))
        pytest.fail(_fault[0] + "\n" + str(e.stderr)[-3000:], pytrace=False)
    if r.returncode < 0 or r.returncode in (134, 139):
        _fault.append("the child of %s ended with status %d" % (name, r.returncode))
        pytest.fail(_fault[0] + "\n" + r.stderr[-3000:], pytrace=False)
    assert r.returncode == 0, r.stderr[-3000:]
    docs = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(docs) == 1, r.stdout[-2000:]
    return json.loads(docs[0]), r.stderr[-3000:]


@pytest.mark.parametrize("name", ab.CASE_SWITCHES)
def test_switch_flipped_runs_its_other_path_within_the_default_bounds(name, gpu):
    sw = ab.SWITCHES[name]
    doc, stderr = _run_child(name)
    print(json.dumps(doc["observable"]), doc["seconds"], "s")
    assert doc["switch"] == name and doc["flip"] == sw["flip"]
    obs = doc["observable"]
    # (a) the switch changed something
    if sw["group"] == "conv":
        assert obs["matches_pinned"], (obs.get("not_as_pinned"), stderr)
        assert obs.get("stats_rows_as_expected", True), (obs, stderr)
        if not sw["no_observable"]:
            assert obs["changed_keys"] > 0 and all(n > 0 for n in obs["cases_changed"].values()), (obs, stderr)
    elif sw["group"] == "tail" and not sw["no_observable"]:
        assert all(o["changed"] for o in obs.values()), (obs, stderr)
    elif sw["group"] == "ln_cf":
        assert all(o["backward_pair_supported"] == 0 for o in obs.values()), (obs, stderr)
    elif sw["group"] == "pointwise":
        assert all(o["as_expected"] for o in obs.values()), (obs, stderr)
    # (b) every check ran something and stayed inside its bound
    assert doc["checks"], stderr
    bad = [c for c in doc["checks"] if not c["ok"]]
    assert not bad, (bad, stderr)
    assert any(c["err"] is not None for c in doc["checks"]), "nothing was launched"
    # (c) no launch refused after its query had said yes
    assert not doc["violations"], (doc["violations"], stderr)
