"""The refusals of the two 1-D engines' raw entries (wt_signals_*, wt_along_*: wt_lines_host.h under wt_signals.hip and
wt_along.hip), byte for byte, in the manner of tests/test_gpu_batch_core.py.

A fixed list of calls, every one an argument error that the library refuses by return code BEFORE any launch or copy:
on a signal stack of 3 signals x 8 samples with max_level 2 and on axis stacks of capacity 6 with N = 8, with planes and
without, each in float32 and float64 - the create rules, the signal ranges, the levels, the entries called out of order,
n_den and its tables, null pointers, pitches and strides, chunks beyond the capacity.  A stack walks through its states
by VALID calls only (upload, decompose, denoise of zeros); the refusals listed under a state leave it as it is.
tests/test_gpu_lines_core.json holds (stack, state, entry, arguments) -> (exception class, message) as the commit
BEFORE the shared host core answered them:

    python tests/test_gpu_lines_core.py --record          (on that commit's library; rewrites the table)

As a test the module replays the list and requires the recorded class and message for every call; a call missing from
the table, or one the library accepts, fails.  Several calls hold two errors at once: they pin the ORDER of the checks."""
import ctypes as _c
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TABLE = os.path.splitext(os.path.abspath(__file__))[0] + ".json"
M, N, ML = 3, 8, 2              # the signal stack
CAP, NO, NI = 6, 2, 3           # the axis stacks: capacity, and the chunk (NO, N, NI) they hold
B3 = 1

NUL = ["null", 0]
BUF = ["buffer", 8 * (ML + 1) * CAP * N]        # a host block no smaller than anything a valid call would move
OUT = ["handle out", 0]
def D(*v): return ["double[]", list(v)]         # noqa: E704
T2 = D(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)      # thresholds of up to 6 signals x 2 planes; the weights take its head


def creates():
    """[(entry, [arguments after the context])]: no stack comes of any of them"""
    c = []
    add = lambda e, *a: c.append((e, list(a)))
    for isz, past in ((4, 8193), (8, 4097)):
        add("wt_signals_create", 0, N, B3, ML, isz, OUT)
        add("wt_signals_create", -1, N, B3, ML, isz, OUT)
        add("wt_signals_create", M, N, 99, ML, isz, OUT)
        add("wt_signals_create", M, N, B3, 0, isz, OUT)
        add("wt_signals_create", M, N, B3, 25, isz, OUT)
        add("wt_signals_create", M, past, B3, ML, isz, OUT)
        add("wt_signals_create", M, 0, B3, ML, isz, OUT)
        add("wt_signals_create", M, N, B3, ML, isz, NUL)
        for planes in (1, 0):
            add("wt_along_create", 0, N, B3, ML, isz, planes, OUT)
            add("wt_along_create", (1 << 30) + 1, N, B3, ML, isz, planes, OUT)
            add("wt_along_create", CAP, N, 99, ML, isz, planes, OUT)
            add("wt_along_create", CAP, N, B3, 0, isz, planes, OUT)
            add("wt_along_create", CAP, N, B3, 25, isz, planes, OUT)
            add("wt_along_create", CAP, 513, B3, ML, isz, planes, OUT)
            add("wt_along_create", CAP, 0, B3, ML, isz, planes, OUT)
            add("wt_along_create", CAP, N, B3, ML, isz, planes, NUL)
    add("wt_signals_create", M, N, B3, ML, 2, OUT)
    add("wt_along_create", CAP, N, B3, ML, 2, 1, OUT)
    add("wt_signals_create", 0, N, B3, ML, 2, OUT)              # (two errors: the order)
    add("wt_signals_create", 0, N, B3, ML, 4, NUL)
    add("wt_along_create", 0, N, 99, ML, 4, 1, OUT)
    add("wt_along_create", 0, N, B3, ML, 4, 1, NUL)
    return c


def signal_calls(state):
    """[(entry, [arguments after the handle])] on a signal stack that is "null" (no handle), "fresh" or "decomposed"
    (signals uploaded, wt_signals_decompose(M, ML) done)"""
    c = []
    add = lambda e, *a: c.append(("wt_signals_" + e, list(a)))
    if state == "null":
        add("info", ["int64 out", 6])
        add("upload", 0, 1, BUF)
        add("decompose", 1, 1)
        add("abs_median", 1, BUF)
        add("denoise_sum", 1, 0, NUL, NUL, 1)
        add("download_planes", 0, 1, BUF)
        add("download_sum", 0, 1, BUF)
        add("upload", 0, 1, NUL)                                # (two errors: the order)
        return c
    add("info", NUL)
    for first, count in ((0, 0), (0, M + 1), (-1, 1), (M, 1), (1, M), (-1, 0)):
        add("upload", first, count, BUF)
        add("download_planes", first, count, BUF)
        add("download_sum", first, count, BUF)
        add("upload", first, count, NUL)                        # (two errors: the order)
        add("download_planes", first, count, NUL)
    for count in (0, M + 1, -1):
        add("decompose", count, ML)
        add("decompose", count, 0)                              # (two errors: the order)
        add("abs_median", count, BUF)
        add("abs_median", count, NUL)
        add("denoise_sum", count, 1, T2, T2, 1)
        add("denoise_sum", count, -1, NUL, NUL, 1)
    for level in (0, ML + 1, -1, 25):
        add("decompose", M, level)
    add("upload", 0, M, NUL)
    add("download_planes", 0, M, NUL)
    add("download_sum", 0, M, NUL)
    add("abs_median", M, NUL)
    if state == "fresh":        # nothing transformed yet
        add("abs_median", M, BUF)
        add("denoise_sum", M, 1, T2, T2, 1)
        add("denoise_sum", M, 0, NUL, NUL, 1)
        add("denoise_sum", M, -1, NUL, NUL, 1)                  # (two errors: the order)
        add("download_planes", 0, M, BUF)
    else:
        for n_den in (-1, ML + 2, 17):
            add("denoise_sum", M, n_den, T2, T2, 1)
            add("denoise_sum", M, n_den, NUL, NUL, 1)           # (two errors: the order)
        add("denoise_sum", M, 1, NUL, T2, 1)
        add("denoise_sum", M, 1, T2, NUL, 1)
        add("denoise_sum", M, ML + 1, NUL, NUL, 0)
    return c


def along_calls(state, planes):
    """[(entry, [arguments after the handle])] on an axis stack with planes or without that is "null", "fresh",
    "loaded" (a chunk of NO x NI signals uploaded) or "done" (with planes: wt_along_decompose(ML); without:
    wt_along_denoise(ML, 0 thresholds))"""
    c = []
    add = lambda e, *a: c.append(("wt_along_" + e, list(a)))
    if state in ("null", "fresh"):        # every entry before any upload
        add("decompose", ML)
        add("abs_median", BUF)
        add("denoise", ML, 1, T2, T2, 1)
        add("download_planes", BUF, NI, NO * N * NI)
        add("download_sum", BUF, NI)
        add("decompose", 0)                                     # (two errors: the order)
        add("abs_median", NUL)
        add("denoise", 0, -1, NUL, NUL, 1)
        add("download_planes", NUL, 0, -1)
        add("download_sum", NUL, 0)
        add("upload", NO, NI, NUL, NI)
        add("info", ["int64 out", 8] if state == "null" else NUL)
        if state == "null":
            add("upload", NO, NI, BUF, NI)
            return c
    # upload: chunks that are no chunk of the stack, pitches below a row
    for no, ni in ((0, NI), (NO, 0), (-1, NI), (CAP + 1, 1), (1, CAP + 1), (NO + 1, NI), (1 << 16, 1 << 16)):
        add("upload", no, ni, BUF, max(ni, 0))
        add("upload", no, ni, BUF, -1)                          # (two errors: the order)
        add("upload", no, ni, NUL, ni)
    add("upload", NO, NI, BUF, NI - 1)
    add("upload", NO, NI, BUF, -1)
    if state == "fresh":
        return c
    add("abs_median", NUL)
    add("download_planes", NUL, NI, NO * N * NI)
    add("download_sum", NUL, NI)
    if planes:
        for level in (0, ML + 1, -1, 25):
            add("decompose", level)
        add("denoise", ML, 0, NUL, NUL, 1)
        add("denoise", 0, -1, NUL, NUL, 1)                      # (two errors: the order)
        add("download_sum", BUF, NI)
        add("download_sum", BUF, NI - 1)                        # (two errors: the order)
        if state == "loaded":
            add("download_planes", BUF, NI, NO * N * NI)
            add("download_planes", BUF, NI - 1, -1)             # (two errors: the order)
        else:
            add("download_planes", BUF, NI - 1, NO * N * NI)
            add("download_planes", BUF, 0, NO * N * NI)
            add("download_planes", BUF, NI, -1)
            add("download_planes", BUF, NI - 1, -1)
            add("download_planes", NUL, NI - 1, -1)             # (two errors: the order)
    else:
        add("decompose", ML)
        add("decompose", 0)                                     # (two errors: the order)
        add("download_planes", BUF, NI, NO * N * NI)
        for level in (0, ML + 1, -1, 25):
            add("denoise", level, 0, NUL, NUL, 1)
            add("denoise", level, -1, NUL, NUL, 1)              # (two errors: the order)
        for n_den in (-1, ML + 1, 17):
            add("denoise", ML, n_den, T2, T2, 1)
            add("denoise", ML, n_den, NUL, NUL, 1)              # (two errors: the order)
        add("denoise", 1, 2, T2, T2, 1)
        add("denoise", ML, 1, NUL, T2, 1)
        add("denoise", ML, 1, T2, NUL, 1)
        add("denoise", ML, ML, NUL, NUL, 0)
        if state == "loaded":
            add("download_sum", BUF, NI)
            add("download_sum", BUF, NI - 1)                    # (two errors: the order)
        else:
            add("download_sum", BUF, NI - 1)
            add("download_sum", BUF, 0)
            add("download_sum", NUL, NI - 1)                    # (two errors: the order)
    return c


def listed():
    """[(stack, state, entry, arguments)] of every call, in the order they are made"""
    out = [("none", "create", e, a) for e, a in creates()]
    out += [("signals", "null", e, a) for e, a in signal_calls("null")]
    out += [("along", "null", e, a) for e, a in along_calls("null", True)]
    for t in ("f32", "f64"):
        out += [("signals " + t, st, e, a) for st in ("fresh", "decomposed") for e, a in signal_calls(st)]
        for planes in (True, False):
            name = f"along {t} {'planes' if planes else 'sum'}"
            out += [(name, st, e, a) for st in ("fresh", "loaded", "done") for e, a in along_calls(st, planes)]
    return out


def key(stack, state, entry, args):
    return json.dumps([stack, state, entry, args])


def _convert(a, keep):
    if not isinstance(a, list):
        return a
    kind, v = a
    if kind == "null":
        return None
    if kind == "handle out":
        obj = _c.c_void_p()
        keep.append(obj)
        return _c.byref(obj)
    if kind == "int64 out":
        obj = (_c.c_int64 * v)()
    elif kind == "buffer":
        obj = (_c.c_char * v)()
        keep.append(obj)
        return _c.c_void_p(_c.addressof(obj))
    else:
        obj = (_c.c_double * len(v))(*v)
    keep.append(obj)
    return obj


def answers():
    """{key: [exception class name or None, message]} of every listed call on this library"""
    from wavelets_amd import _lib as L
    lib, ctx = L.load(), L.default_context()
    out = {}

    def refuse(stack, state, handle, calls):
        for entry, args in calls:
            keep = []
            head = [ctx._h] if state == "create" else [handle]
            try:
                L.check(getattr(lib, entry)(*head, *[_convert(a, keep) for a in args]))
                out[key(stack, state, entry, args)] = [None, ""]
                made = [o for o in keep if isinstance(o, _c.c_void_p) and o.value]
                assert not made, f"{entry}{args} made a stack"
            except L.WatrooHipError as e:
                out[key(stack, state, entry, args)] = [type(e).__name__, str(e)]

    def valid(rc):
        L.check(rc)

    refuse("none", "create", None, creates())
    refuse("signals", "null", None, signal_calls("null"))
    refuse("along", "null", None, along_calls("null", True))
    for t, dtype in (("f32", np.float32), ("f64", np.float64)):
        isz = np.dtype(dtype).itemsize
        h = _c.c_void_p()
        valid(lib.wt_signals_create(ctx._h, M, N, B3, ML, isz, _c.byref(h)))
        try:
            refuse("signals " + t, "fresh", h, signal_calls("fresh"))
            zeros = np.zeros((M, N), dtype)
            valid(lib.wt_signals_upload(h, 0, M, _c.c_void_p(zeros.ctypes.data)))
            valid(lib.wt_signals_decompose(h, M, ML))
            refuse("signals " + t, "decomposed", h, signal_calls("decomposed"))
        finally:
            ctx.sync()
            valid(lib.wt_signals_destroy(h))
        for planes in (True, False):
            name = f"along {t} {'planes' if planes else 'sum'}"
            h = _c.c_void_p()
            valid(lib.wt_along_create(ctx._h, CAP, N, B3, ML, isz, int(planes), _c.byref(h)))
            try:
                refuse(name, "fresh", h, along_calls("fresh", planes))
                zeros = np.zeros((NO, N, NI), dtype)
                valid(lib.wt_along_upload(h, NO, NI, _c.c_void_p(zeros.ctypes.data), NI))
                refuse(name, "loaded", h, along_calls("loaded", planes))
                if planes:
                    valid(lib.wt_along_decompose(h, ML))
                else:
                    valid(lib.wt_along_denoise(h, ML, 0, None, None, 1))
                refuse(name, "done", h, along_calls("done", planes))
            finally:
                ctx.sync()
                valid(lib.wt_along_destroy(h))
    return out


def test_the_1d_engines_refuse_what_they_refused_in_their_words():
    table = json.load(open(TABLE))
    keys = [key(*c) for c in listed()]
    assert table and len(set(keys)) == len(keys) > 400
    missing = [k for k in keys if k not in table]
    assert not missing, f"{len(missing)} listed calls are not in the recorded table, first: {missing[0]}"
    got = answers()
    accepted = [k for k in keys if got[k][0] is None]
    assert not accepted, f"{len(accepted)} calls were not refused, first: {accepted[0]}"
    wrong = [(k, got[k], table[k]) for k in keys if got[k] != table[k]]
    assert not wrong, f"{len(wrong)} refusals changed, first: {wrong[0][0]}: {wrong[0][1]} != recorded {wrong[0][2]}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_lines_core.py --record [--out FILE]")
    got = answers()
    accepted = [k for k, v in got.items() if v[0] is None]
    if accepted:
        sys.exit("not refused, so not an argument error - take it off the list:\n" + "\n".join(accepted))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else TABLE
    json.dump(got, open(path, "w"), indent=0, sort_keys=True)
    print(f"{len(got)} refusals recorded in {path}")
