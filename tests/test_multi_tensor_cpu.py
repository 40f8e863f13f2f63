"""CPU: every multi-tensor entry (csrc/multi_tensor.h) checks its WHOLE table before its first launch.  A table of 100 tensors is more than two
launches' worth (YOLO_MT_MAX = 48); a bad entry at index 48 or 99 lies behind the first launch, so an entry that checked while it batched would
launch the first 48 tensors -- without a device that launch fails with HIP's own code, with one it would have updated them -- before it got
there.  The calls here are all refused on the host: the addresses are made up and never dereferenced."""

import ctypes
import re

import pytest

COUNT, N = 100, 16
BASE = {name: 0x1000000 * (k + 1) for k, name in enumerate("abcd")}       # one made-up array per field, 16-B aligned, tensors 256 B apart
NULL, NEGATIVE, MISALIGNED = "null pointer", "negative size", "pointer + 4"


def _lib():
    from yolo import _hip
    if not _hip.available():
        import __graft_entry__ as g
        g.build()
    return _hip.lib()


def _fields(i, bad):
    """(a, b, c, d, n) of tensor i: four addresses and the size; `bad` spoils field b"""
    a, b, c, d = (BASE[k] + 256 * i for k in "abcd")
    if bad == NULL:
        b = None
    if bad == MISALIGNED:
        b += 4
    return a, b, c, d, (-1 if bad == NEGATIVE else N)


def _call(entry, where, bad):
    from yolo import _hip
    L = _lib()
    rows = [_fields(i, bad if i == where else None) for i in range(COUNT)]
    acc, scratch = 0x9000000, 0xA000000
    if entry == "yolo_adam_step_multi":
        tab = (_hip.AdamTensor * COUNT)(*[_hip.AdamTensor(a, b, c, d, None, n) for a, b, c, d, n in rows])      # b: the gradient
        return L.yolo_adam_step_multi(tab, COUNT, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.0, None, None)
    if entry == "yolo_sgd_step_multi":
        tab = (_hip.SgdTensor * COUNT)(*[_hip.SgdTensor(a, b, c, None, n) for a, b, c, _, n in rows])           # b: the gradient
        return L.yolo_sgd_step_multi(tab, COUNT, 0.1, 0.9, 0.0, 0.0, 0, 0, None, 0.0, None, None)
    if entry == "yolo_ema_update_multi":
        tab = (_hip.EmaTensor * COUNT)(*[_hip.EmaTensor(a, b, n) for a, b, _, _, n in rows])                    # b: the parameter
        return L.yolo_ema_update_multi(tab, COUNT, 0.1, None, None)
    if entry == "yolo_grad_accum_multi":
        tab = (_hip.AccumTensor * COUNT)(*[_hip.AccumTensor(a, b, c, n) for a, b, c, _, n in rows])             # b: x
        return L.yolo_grad_accum_multi(tab, COUNT, 0.5, None, None)
    g = (ctypes.c_void_p * COUNT)(*[r[1] for r in rows])
    n = (ctypes.c_long * COUNT)(*[r[4] for r in rows])
    if entry == "yolo_sumsq_f32_multi":
        return L.yolo_sumsq_f32_multi(g, n, COUNT, acc, None)
    assert entry == "yolo_sumsq_f32_multi_fixed"
    return L.yolo_sumsq_f32_multi_fixed(g, n, COUNT, scratch, 1000, acc, None)


ENTRIES = ["yolo_adam_step_multi", "yolo_sumsq_f32_multi", "yolo_sgd_step_multi", "yolo_ema_update_multi", "yolo_grad_accum_multi",
           "yolo_sumsq_f32_multi_fixed"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_bad_tensor_behind_the_first_launch_refuses_the_whole_call(entry):
    from yolo import _hip
    L = _lib()
    want = {NULL: _hip.E_ARG, NEGATIVE: _hip.E_ARG, MISALIGNED: _hip.E_UNSUPPORTED}
    for where in (48, 99):
        for bad, code in want.items():
            rc = _call(entry, where, bad)
            msg = L.yolo_hip_last_error().decode(errors="replace")
            assert rc == code, f"{entry}: {bad} at {where}: code {rc} ({msg})"
            assert entry in msg and re.search(rf"\b{where}\b", msg), f"{entry}: {bad} at {where}: {msg}"
