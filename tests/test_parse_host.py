"""Host side of the airway tree parsing: tests/parse_oracle.py reproduces every array the reference produced
(tests/golden/parse_known.npz, recorded by scripts/make_golden_parse.py), the refinement on label statistics agrees with it,
and the C ABI declares and exports the new entry points."""
import os
import re
import subprocess

import numpy as np
import pytest

import parse_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "parse_known.npz")
ENTRY_POINTS = ("seunet_skeleton_branches_workspace_bytes", "seunet_skeleton_branches", "seunet_parse_assign_workspace_bytes",
                "seunet_parse_assign", "seunet_label_stats_max_num", "seunet_label_stats", "seunet_relabel")


def cases():
    z = np.load(GOLDEN)
    return [{k[len(f"case{i}_"):]: z[k] for k in z.files if k.startswith(f"case{i}_")} for i in range(int(z["ncase"]))]


CASES = cases()


def test_fixture_holds_the_cases_the_tests_rely_on():
    assert max(int(c["rounds"]) for c in CASES) >= 3
    assert any(int(c["num0"]) > int(c["num"]) for c in CASES)
    assert any(any(n % 64 for n in c["label"].shape) for c in CASES) and any(c["label"].shape[2] > 128 for c in CASES)
    assert any(not np.array_equal(po.skeleton_parsing(c["skeleton"], mode="constant")[1], c["cd"]) for c in CASES)   # the mirror matters


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_oracle_reproduces_the_reference(ci):
    c = CASES[ci]
    got = po.tree_parsing(c["label"], c["skeleton"])
    assert np.array_equal(got["skeleton_parse"], c["skeleton_parse"])
    assert np.array_equal(got["cd"], c["cd"]) and got["num0"] == int(c["num0"])
    assert np.array_equal(got["parsing0"], c["parsing0"])
    assert np.array_equal(got["counts0"], c["counts0"]) and np.array_equal(got["ad0"], c["ad0"])
    assert got["trachea0"] == int(c["trachea0"])
    assert got["rounds"] == int(c["rounds"]) and got["num"] == int(c["num"])
    assert np.array_equal(got["parsing"], c["parsing"])
    assert got["parsing"].dtype == np.int32 and got["cd"].dtype == np.int32


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_refinement_on_statistics_equals_the_reference(ci):
    """prep.refine_labels follows the loop on the counts and the adjacency of the unrefined volume alone."""
    from seunet_amd import prep
    c = CASES[ci]
    num0 = int(c["num0"])
    counts = np.concatenate([[0], c["counts0"]])
    adj = np.zeros((num0 + 1, num0 + 1), dtype=bool)
    adj[1:, 1:] = c["ad0"] != 0
    lut, num, rounds = prep.refine_labels(counts, adj, num0)
    assert num == int(c["num"]) and rounds == int(c["rounds"])
    assert np.array_equal(lut[c["parsing0"].astype(np.int64)], c["parsing"])


def test_entry_points_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seunet_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(seunet_[a-z0-9_]+)\s*\(", text))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    from seunet_amd import _lib
    assert set(ENTRY_POINTS) <= set(_lib.PROTOTYPES)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the library is not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (seunet_[a-z0-9_]+)", out))
    assert set(ENTRY_POINTS) <= exported, sorted(set(ENTRY_POINTS) - exported)
    lib = _lib.load()
    assert lib.seunet_label_stats_max_num() >= 4095
    assert lib.seunet_skeleton_branches_workspace_bytes(4, 5, 6) > 0 and lib.seunet_parse_assign_workspace_bytes(4, 5, 6) > 0
