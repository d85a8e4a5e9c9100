"""What lrn_set_option does with a key and a value, seen without a device through lrn_dbg_option_probe: the return code, the
error text, the bytes of the options struct that differ from the defaults, and the fields of the context an option may touch.

tests/golden/option_semantics.json holds one record per key and probe value.  It was recorded on the commit before the option
table (csrc/options.h) existed, from the if-chain lrn_set_option was then, with this module and the same probe; the keys came
from the chain's own source text.  `python tests/option_cases.py` records it again from the library as built, with the keys
lrn_dbg_option_name enumerates -- the file must come out unchanged.

The byte image is compared, not a field by name: a name -> field map written for the test would share its mistakes with the
table."""
import ctypes as C
import json
import math
import os
import struct
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "option_semantics.json")

PROBE_VALUES = [-2.0, -1.0, 0.0, 0.5, 1.0, 2.0, 3.0, 17.0, 127.0, 200.0, 1.0e6, 1.0e10]
WATCHED = ["hop_version", "profile", "lz_res_limit", "lz_wh_left", "lz_wh_fired", "lz_wh_run", "lz_wh_step", "lz_wh_wg",
           "shard_bs_opt", "shard_bs", "t_cap", "p_cap", "timing_entries", "count_entries"]
SKIPPED = ["comm_fail_ensure", "detect_release"]          # their action needs a communicator / a device: not probed
TEST_HOOKS = ["lz_test_withhold", "comm_fail_ensure"]
# the keys that live on the context: what lrn_create leaves them at (None: an action, no state)
CONTEXT_DEFAULTS = {"profile": 0.0, "lz_res_limit": 2000000.0, "lz_test_withhold": 0.0, "shard_bs": 0.0, "reset_timing": None,
                    "comm_fail_ensure": None, "detect_release": None}


def probe(lib, key, value):
    """-> (rc, error text, bytes of the options struct, watched fields) of lrn_set_option(key, value); key None: the start"""
    rc, size, w, msg = C.c_int(0), C.c_int(0), (C.c_int64 * len(WATCHED))(), C.create_string_buffer(1024)
    buf = C.create_string_buffer(4096)
    st = lib.lrn_dbg_option_probe(None if key is None else key.encode(), float(value), C.byref(rc), msg, len(msg), buf, len(buf),
                                  C.byref(size), w)
    assert st == 0 and 0 < size.value <= len(buf), (key, value, st, size.value)
    return rc.value, msg.value.decode(), buf.raw[:size.value], list(w)


def changed(image, defaults):
    """the maximal byte ranges in which image differs from defaults: [[offset, hex of the new bytes], ...]"""
    assert len(image) == len(defaults)
    out, i, n = [], 0, len(image)
    while i < n:
        if image[i] == defaults[i]:
            i += 1
            continue
        j = i
        while j < n and image[j] != defaults[j]:
            j += 1
        out.append([i, image[i:j].hex()])
        i = j
    return out


def record_of(lib, key, value, defaults):
    rc, err, image, watched = probe(lib, key, value)
    return [repr(float(value)), rc, err, changed(image, defaults), watched]


def _default_of(lib, key, records, defaults):
    """the value that leaves the options struct at its defaults, found by trial: the integers and the double that overlap the
    first byte a probe changed, the double first.  None: the key stores nothing in the options struct"""
    offs = [r[3][0][0] for r in records if r[1] == 0 and r[3]]
    if not offs:
        return None
    o = min(offs)
    cands = []
    if (o & ~7) + 8 <= len(defaults):
        cands += [struct.unpack_from("<d", defaults, o & ~7)[0], float(struct.unpack_from("<q", defaults, o & ~7)[0])]
    cands.insert(1, float(struct.unpack_from("<i", defaults, o & ~3)[0]))
    for v in cands:
        if math.isfinite(v) and abs(v) < 2.0 ** 31:          # (an int field takes any of them)
            rc, _err, image, _w = probe(lib, key, v)
            if rc == 0 and image == defaults:
                return v
    raise AssertionError(f"{key}: no value sets the default back")


def record(lib, keys, nan_keys=(), no_huge_keys=()):
    """keys: every key of lrn_set_option; nan_keys: those whose code tests for NaN; no_huge_keys: those that cast the value to
    int unguarded (1e10 does not fit: undefined, not probed)"""
    _rc, _err, defaults, start = probe(lib, None, 0.0)
    out = {"opt_size": len(defaults), "watched": WATCHED, "start": start, "skipped": SKIPPED, "test_hooks": TEST_HOOKS, "keys": {}}
    for key in keys:
        if key in SKIPPED:
            continue
        values = [v for v in PROBE_VALUES if not (v == 1.0e10 and key in no_huge_keys)]
        if key in nan_keys:
            values.append(float("nan"))
        recs = [record_of(lib, key, v, defaults) for v in values]
        default = CONTEXT_DEFAULTS[key] if key in CONTEXT_DEFAULTS else _default_of(lib, key, recs, defaults)
        ok = [r for r in recs if r[1] == 0]
        accepted = next((r for r in ok if r[3] or r[4] != start), ok[0])[0]
        out["keys"][key] = {"default": default, "accepted": float(accepted), "records": recs}
    return out


def dump(data, path):
    with open(path, "w") as f:
        f.write('{"opt_size": %d,\n "watched": %s,\n "start": %s,\n "skipped": %s,\n "test_hooks": %s,\n "keys": {\n' % (
            data["opt_size"], json.dumps(data["watched"]), json.dumps(data["start"]), json.dumps(data["skipped"]),
            json.dumps(data["test_hooks"])))
        items = sorted(data["keys"].items())
        for n, (key, e) in enumerate(items):
            f.write('  %s: {"default": %s, "accepted": %s, "records": [\n' % (json.dumps(key), json.dumps(e["default"]),
                                                                             json.dumps(e["accepted"])))
            f.write(",\n".join("    " + json.dumps(r) for r in e["records"]))
            f.write("]}%s\n" % ("," if n + 1 < len(items) else ""))
        f.write(" }}\n")


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def enumerated_keys(lib):
    keys, i = [], 0
    while True:
        name = lib.lrn_dbg_option_name(i)
        if name is None:
            return keys
        keys.append(name.decode())
        i += 1


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import loraine_jl_amd
    lib_ = loraine_jl_amd.load_library()
    gold = load()
    nan_keys_ = [k for k, e in gold["keys"].items() if any(r[0] == "nan" for r in e["records"])]
    no_huge_ = [k for k, e in gold["keys"].items() if not any(r[0] == repr(1.0e10) for r in e["records"])]
    dump(record(lib_, enumerated_keys(lib_), nan_keys_, no_huge_), sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
