"""What the tests of the five replay entries (tsd_debug_gemm_run, tsd_debug_norm_run, tsd_debug_attn_run, tsd_debug_chain_run,
tsd_debug_elem_run: csrc/api_replay.cpp) share: the
fill patterns of the guarded operands, the enum reader of include/tsd.h, the sizing-only call, the run on caller operands, and the two
statements about an output's bytes that every family makes (a refused launch wrote nothing; the pitch gaps still hold the fill)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "tsd.h")
NAN16 = np.array([0x7E5A], np.uint16).view(np.float16)[0]
NAN32 = np.array([0x7FC5A5A5], np.uint32).view(np.float32)[0]
_i64p = C.POINTER(C.c_int64)
_SLOTS = 32          # no entry has more operand slots or info fields


def f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def bits_f32(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def header():
    """include/tsd.h without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def enum(txt, name):
    body = re.search(r"enum\s+" + name + r"\s*\{(.*?)\}", txt, re.S).group(1)
    out, v = {}, 0
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        if "=" in item:
            k, val = (s.strip() for s in item.split("="))
            v = int(val, 0)
        else:
            k = item
        out[k] = v
        v += 1
    return out


def enums(txt, names):
    """{prefix: enum name} -> one dict per enum, in order, the prefix stripped from its keys."""
    return [{k[len(p):]: v for k, v in enum(txt, e).items()} for p, e in names.items()]


def version(txt, name):
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", txt).group(1))


def lib():
    from tsd._lib import lib as load
    return load()


def _p(a):
    return None if a is None else a.ctypes.data_as(_i64p)


def size(fn_name, d, n=None, info=None, ctx=None, extra=()):
    """The sizing-only call (no operands, no device): (status, extent per slot index).  info, when given, receives the plan."""
    d = np.ascontiguousarray(d, np.int64)
    ext = np.zeros(_SLOTS, np.int64)
    rc = getattr(lib(), fn_name)(ctx, _p(d), len(d) if n is None else n, *extra, None, None, _p(ext), _p(info))
    return rc, ext


def run(fn_name, ctx, d, ops, slots, inputs, outputs, dtype_of, extents, extra=(), unsizable_ok=False):
    """Size d, hold the entry's extents against the reference module's, run it on ops: (status, {output slot: flat array}, info).
    unsizable_ok: a descriptor the entry cannot size gives (status, None, None) instead of failing."""
    d = np.ascontiguousarray(d, np.int64)
    rc, ext = size(fn_name, d, ctx=ctx.h, extra=extra)
    if rc != 0 and unsizable_ok:
        return rc, None, None
    assert rc == 0, lib().tsd_last_error().decode()
    want = extents(d)
    assert slots["COUNT"] <= _SLOTS
    assert {s: int(ext[slots[s]]) for s in want} == want, f"{fn_name} and the reference module size the operands differently"
    ins = (C.c_void_p * slots["COUNT"])()
    for s in inputs:
        if want[s]:
            assert ops[s].size == want[s] and ops[s].dtype == dtype_of(s, d) and ops[s].flags.c_contiguous, s
            ins[slots[s]] = ops[s].ctypes.data
    outs, outp = {}, (C.c_void_p * len(outputs))()
    for i, s in enumerate(outputs):
        if want[s]:
            outs[s] = np.empty(want[s], dtype_of(s, d))
            outp[i] = outs[s].ctypes.data
    info = np.zeros(_SLOTS, np.int64)
    rc = getattr(lib(), fn_name)(ctx.h, _p(d), len(d), *extra, ins, outp, _p(ext), _p(info))
    return rc, outs, info


def assert_untouched(outs, what):
    """Every output still holds the fill, byte for byte."""
    for s, o in outs.items():
        pat = NAN32 if o.dtype == np.float32 else NAN16
        assert np.array_equal(o.view(np.uint8), np.full_like(o, pat).view(np.uint8)), f"{what}: {s} was written"


def assert_gaps_hold_fill(out, logical_index, what):
    """The elements of the fp16 (or fp32) output that are no logical element still hold the fill."""
    gap = np.ones(out.size, bool)
    gap[np.asarray(logical_index).ravel()] = False
    if out.dtype == np.float32:
        assert (out.view(np.uint32)[gap] == NAN32.view(np.uint32)).all(), f"{what}: a pitch gap was written"
        return
    assert (out.view(np.uint16)[gap] == NAN16.view(np.uint16)).all(), f"{what}: a pitch gap was written"


def ctx_with(tsd_mod, gpu_ctx, monkeypatch, var, value):
    """A context created with an option in the environment (read once, by tsd_ctx_create); the environment is restored at once."""
    monkeypatch.setenv(var, str(value))
    c = tsd_mod.Context(gpu_ctx.device)
    monkeypatch.delenv(var)
    return c
