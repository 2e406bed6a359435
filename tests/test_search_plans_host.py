"""CPU: the workspace sizes of the four scan-based search calls over a grid of shapes, against recorded values.

The plans behind mmr_search_workspace_bytes, mmr_range_workspace_bytes, mmr_sweep_workspace_bytes and
mmr_deep_topk_workspace_bytes decide where every region of a caller's workspace lies.  A change to the host front end
(csrc/scan_host.h) or to a plan must leave every total as it was: tests/golden/search_plan_sizes.json holds the totals
of a known build, and every cell of the grid is compared with it.

Recording (on a checkout of the commit whose sizes are the reference, after building its library):

    python tests/test_search_plans_host.py --record [--commit HASH] [--out FILE]

writes the JSON; its head notes the recording mode and the commit.  The size functions run on the host alone."""
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "search_plan_sizes.json")

# N crosses the 256-tile switch of the task plan for 32-row (8192) and 16-row (4096 < 8191) tiles; Q reaches both sides of
# the queries-per-pass limit (64, 128, 256) of every E x dtype
NS = (0, 1, 31, 32, 33, 8191, 8192, 8193, 50003, 100000, 1000000)
QS = (1, 37, 64, 65, 128, 129, 200, 256, 257)
ES = (128, 256, 512, 768)
DTYPES = (0, 1, 2)          # MMR_F32, MMR_BF16, MMR_F16
GIVEN = (0, 1)              # gallery_hi_given / split_given
TOPK_KS = (10, 64)          # with and without the MFMA fast path (k + 6 <= 32)
CAND_CAP, SWEEP_T, DEEP_K, TILE_CAP, SURV_CAP = 4096, 50, 100, 4096, 8192


def _cells(name):
    """(key, arguments) of every cell of one function's grid, in a fixed order."""
    if name == "search":      # no dtype argument: the size covers the bf16 and the fp32 plan
        for n, e, q, k in itertools.product(NS, ES + (1024,), QS, TOPK_KS):
            yield f"N={n} E={e} Q={q} k={k}", (n, e, q, k)
        return
    for n, e, q, dt, given in itertools.product(NS, ES, QS, DTYPES, GIVEN):
        key = f"N={n} E={e} Q={q} dtype={dt} given={given}"
        if name == "range":
            yield key, (n, e, q, CAND_CAP, dt, given)
        elif name == "sweep":
            yield key, (n, e, q, SWEEP_T, CAND_CAP, dt, given)
        else:
            yield key, (n, e, q, DEEP_K, TILE_CAP, SURV_CAP, dt, given)


FUNCS = {"search": "mmr_search_workspace_bytes", "range": "mmr_range_workspace_bytes", "sweep": "mmr_sweep_workspace_bytes",
         "deep": "mmr_deep_topk_workspace_bytes"}


def _sizes(L, name):
    f = getattr(L, FUNCS[name])
    return [int(f(*args)) for _, args in _cells(name)]


def _load_lib():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from mmr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        raise RuntimeError(f"{_lib.LIB_PATH} missing: run __graft_entry__.build() first")
    return _lib.lib()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_recording_notes_its_mode_and_commit(recorded):
    assert "--record" in recorded["recorded_by"]
    assert len(recorded["commit"]) >= 7
    assert recorded["grid"] == {"N": list(NS), "Q": list(QS), "E": list(ES), "dtype": list(DTYPES), "given": list(GIVEN),
                                "topk_k": list(TOPK_KS), "cand_cap": CAND_CAP, "T": SWEEP_T, "deep_k": DEEP_K,
                                "tile_cap": TILE_CAP, "surv_cap": SURV_CAP}


@pytest.mark.parametrize("name", list(FUNCS))
def test_workspace_sizes_equal_the_recorded_ones(recorded, name):
    want = recorded["sizes"][name]
    got = _sizes(_load_lib(), name)
    keys = [k for k, _ in _cells(name)]
    assert len(want) == len(got) == len(keys)
    assert any(want) and len(set(want)) > len(NS)           # a real table, not zeros
    diff = [(k, w, g) for k, w, g in zip(keys, want, got) if w != g]
    assert not diff, f"{FUNCS[name]}: {len(diff)} of {len(keys)} cells differ (cell, recorded, now), first: {diff[:5]}"


def _record(argv):
    commit, out = None, GOLDEN
    for i, a in enumerate(argv):
        if a == "--commit":
            commit = argv[i + 1]
        if a == "--out":
            out = argv[i + 1]
    if commit is None:
        import subprocess
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    L = _load_lib()
    doc = {"recorded_by": "python tests/test_search_plans_host.py --record (totals of the library built from `commit`)",
           "commit": commit,
           "grid": {"N": NS, "Q": QS, "E": ES, "dtype": DTYPES, "given": GIVEN, "topk_k": TOPK_KS, "cand_cap": CAND_CAP,
                    "T": SWEEP_T, "deep_k": DEEP_K, "tile_cap": TILE_CAP, "surv_cap": SURV_CAP},
           "order": "itertools.product over N, E (plus 1024 for search), Q, then k (search) or dtype, given",
           "sizes": {name: _sizes(L, name) for name in FUNCS}}
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {out}: " + ", ".join(f"{n} {len(v)}" for n, v in doc["sizes"].items()))


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_search_plans_host.py --record [--commit HASH] [--out FILE]")
    _record(sys.argv[1:])
