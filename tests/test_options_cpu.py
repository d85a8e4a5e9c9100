"""lrn_set_option through the option table (csrc/options.h) does, key by key and value by value, what the if-chain it replaced
did: tests/golden/option_semantics.json was recorded from that chain (option_cases.py says how), and lrn_dbg_option_probe
replays every record on a context that exists on the host only -- return code, error text, changed bytes of the options struct,
watched fields of the context, all exactly.  No GPU."""
import copy

import pytest

import loraine_jl_amd
import option_cases as oc

GOLD = oc.load()
LRN_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    return loraine_jl_amd.load_library()


@pytest.fixture(scope="module")
def defaults(lib):
    rc, err, image, start = oc.probe(lib, None, 0.0)
    assert (rc, err) == (0, "") and len(image) == GOLD["opt_size"] and start == GOLD["start"]
    return image


def mismatches(lib, key, records, defaults):
    """the records of `key` the library does not reproduce"""
    return [(want, got) for want in records for got in [oc.record_of(lib, key, float(want[0]), defaults)] if got != want]


def test_the_enumerated_keys_are_the_recorded_ones(lib):
    keys = oc.enumerated_keys(lib)
    assert len(keys) == len(set(keys))                                       # every key once
    assert sorted(keys) == sorted(list(GOLD["keys"]) + GOLD["skipped"])      # an arm of the chain that was forgotten shows here
    assert lib.lrn_dbg_option_name(-1) is None and lib.lrn_dbg_option_name(len(keys)) is None


@pytest.mark.parametrize("key", sorted(GOLD["keys"]))
def test_every_record_is_reproduced(lib, defaults, key):
    entry = GOLD["keys"][key]
    values = [r[0] for r in entry["records"]]
    assert set(values) >= {repr(v) for v in oc.PROBE_VALUES[:-1]}            # (1e10 only where the cast is guarded)
    assert not mismatches(lib, key, entry["records"], defaults)


def test_an_unknown_key_is_an_argument_error(lib, defaults):
    for key in ("no_such_option", "pair_loca", "pair_local ", ""):
        rc, err, image, watched = oc.probe(lib, key, 1.0)
        assert (rc, err) == (LRN_ERR_ARG, f"unknown option {key}")
        assert image == defaults and watched == GOLD["start"]


def test_the_skipped_keys_are_refused_by_the_probe(lib):
    import ctypes as C
    rc, size, w = C.c_int(0), C.c_int(0), (C.c_int64 * 14)()
    for key in GOLD["skipped"]:
        assert lib.lrn_dbg_option_probe(key.encode(), 1.0, C.byref(rc), None, 0, None, 0, C.byref(size), w) == LRN_ERR_ARG


def test_planted_faults_are_caught(lib, defaults):
    """the comparison sees a side effect that went missing and a value stored in the neighbouring field"""
    records = GOLD["keys"]["matvec_h"]["records"]
    assert not mismatches(lib, "matvec_h", records, defaults)
    hop = oc.WATCHED.index("hop_version")
    flipped = copy.deepcopy(records)
    for r in flipped:
        assert r[4][hop] == -1                        # INVALIDATES_HOP
        r[4][hop] = GOLD["start"][hop]                # ... expected not to happen
    assert len(mismatches(lib, "matvec_h", flipped, defaults)) == len(records)
    moved = copy.deepcopy(records)
    stored = [r for r in moved if r[3]]
    assert stored
    for r in stored:
        r[3][0][0] += 4                               # the int one field further on
    assert len(mismatches(lib, "matvec_h", moved, defaults)) == len(stored)
    caps = copy.deepcopy(GOLD["keys"]["t_batch"]["records"])
    for r in caps:
        assert r[4][oc.WATCHED.index("t_cap")] == 0 and r[4][oc.WATCHED.index("p_cap")] == 0      # RESETS_BATCH_CAPS
        r[4][oc.WATCHED.index("p_cap")] = GOLD["start"][oc.WATCHED.index("p_cap")]
    assert len(mismatches(lib, "t_batch", caps, defaults)) == len(caps)


def test_the_reject_cases_carry_their_texts():
    """what the chain rejected with a message, it still does (the GPU test reads the same records on a real context)"""
    texts = {key: sorted({r[2] for r in e["records"] if r[1] != 0}) for key, e in GOLD["keys"].items()}
    texts = {k: v for k, v in texts.items() if v}
    assert texts == {
        "pair_local": ["pair_local is 0 or 1"], "pair_long": ["pair_long is 0 or 1"], "pair_long_mfma": ["pair_long_mfma is 0 or 1"],
        "pair_local_min": ["pair_local_min is a count of entries >= 1"], "pair_long_min": ["pair_long_min is a count of entries >= 1"],
        "pair_long_split": ["pair_long_split is a count of products >= 1"],
        "pair_long_scratch_mb": ["pair_long_scratch_mb is a size >= 0"],
        "lz_res_limit": [""], "lz_test_withhold": [""], "shard_bs": [""]}


def test_the_table_walk_on_the_host(tmp_path):
    """tests/host/options_walk.cpp: option_apply on a plain LrnOptions, every key of the table with every probe value"""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "options_walk")
    src = os.path.join(root, "tests", "host", "options_walk.cpp")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-w", "-I", os.path.join(root, "loraine.jl_amd", "csrc"), src, "-o", exe],
                   check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout and f"options={len(GOLD['keys']) + len(GOLD['skipped']) - 7} context=7" in out.stdout
