"""Token merging (ToMe for Stable Diffusion, Bolya & Hoffman 2023) in front of self attention: the model table of
`tsd_model_set_token_merge`, the three launches alone, and the scope `generate` / `generate_stream` set a table in.  include/tsd.h
"Token merging" states the semantics.  No reference counterpart."""
import contextlib
import ctypes as C

import numpy as np

from ._lib import check, lib
from .utils import _ctx

MAX_RATIO = 0.75


def token_merge_table(ratio):
    """None | float (level 0) | 4 floats -> the ratio table of `tsd_model_set_token_merge`."""
    if ratio is None:
        return (0.0, 0.0, 0.0, 0.0)
    if isinstance(ratio, (int, float, np.integer, np.floating)):
        return (float(ratio), 0.0, 0.0, 0.0)
    t = tuple(float(v) for v in ratio)
    if len(t) != 4:
        raise ValueError(f"token_merge is a float (the top level's ratio) or 4 ratios, one per level; got {ratio!r}")
    return t


def merged_count(ratio, N):
    """r = 8 floor(ratio N / 8), with ratio rounded to float32 as the library receives it."""
    return 8 * int(np.floor(float(np.float32(ratio)) * N / 8.0))


class _TokenMerge:
    """`set_token_merge` / `token_merge` of the models that have self-attention blocks (Diffusion, ControlNet)."""

    def set_token_merge(self, ratio=None, seed=0):
        """Token merging (`tsd_model_set_token_merge`): a float is the share of the top level's tokens merged in front of its self
        attention, a 4-tuple gives one ratio per level l (token grid LH / 2^l x LW / 2^l); ratios are in [0, 0.75] and a merging level
        needs an even-sided grid of 64 .. 32768 tokens and no window.  seed picks the destination token of every 2 x 2 cell (0: the
        top-left one); set a new seed between steps for a fresh partition per step.  None or zeros turn it off.  State of the model:
        it acts from the next forward on, a step of an open `Session` included (no `upload`, no larger workspace)."""
        t = token_merge_table(ratio)
        check(lib().tsd_model_set_token_merge(self.model.h, None if ratio is None else (C.c_float * 4)(*t), int(seed) & 0xFFFFFFFF))

    @property
    def token_merge(self):
        """(the model's ratio table, a 4-tuple - all zeros = off -, seed)."""
        out, seed = (C.c_float * 4)(), C.c_uint32(0)
        on = lib().tsd_model_token_merge(self.model.h, out, C.byref(seed))
        if on < 0:
            check(on)
        return tuple(float(v) for v in out), int(seed.value)


@contextlib.contextmanager
def token_merge_scope(model, token_merge):
    """`generate(token_merge=...)`: a ratio, 4 ratios or (ratios, seed); the model's previous table is back on every way out."""
    if token_merge is None or not hasattr(model, "set_token_merge"):
        yield
        return
    ratio, seed = token_merge if isinstance(token_merge, (tuple, list)) and len(token_merge) == 2 else (token_merge, 0)
    prev = model.token_merge
    model.set_token_merge(ratio, seed)
    try:
        yield
    finally:
        model.set_token_merge(*prev)


def token_merge_plan(x, H, W, ratio, seed=0, ctx=None):
    """The match and select launches alone (`tsd_token_merge_plan_f16`): x float16 (B, H W, C), C a multiple of 64 ->
    dict(node_max (B, Ns) float32, node_idx (B, Ns), row_of (B, N), start (B, N - r + 1), members (B, N), rows = N - r)."""
    xa = np.ascontiguousarray(x, dtype=np.float16)
    if xa.ndim != 3 or xa.shape[1] != H * W:
        raise ValueError(f"token_merge_plan: x is (B, H W, C) with H W = {H * W}, got {xa.shape}")
    B, N, Cc = xa.shape
    Ns, r = N - N // 4, merged_count(ratio, N) if 0 <= ratio <= MAX_RATIO else 0     # (the library refuses any other ratio)
    out = dict(node_max=np.empty((B, Ns), np.float32), node_idx=np.empty((B, Ns), np.int32), row_of=np.empty((B, N), np.int32),
               start=np.empty((B, max(N - r, 0) + 1), np.int32), members=np.empty((B, N), np.int32))
    check(lib().tsd_token_merge_plan_f16(_ctx(ctx), xa.ctypes.data, B, int(H), int(W), Cc, float(ratio), int(seed) & 0xFFFFFFFF,
                                         *(out[k].ctypes.data for k in ("node_max", "node_idx", "row_of", "start", "members"))))
    out["rows"] = N - r
    return out


def token_merge_rows(x, start, members, ctx=None):
    """The merge launch alone (`tsd_token_merge_rows_f16`): x float16 (B, N, C), start (B, rows + 1), members (B, N) -> (B, rows, C)."""
    xa = np.ascontiguousarray(x, dtype=np.float16)
    st, me = np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(members, dtype=np.int32)
    if xa.ndim != 3 or st.ndim != 2 or me.shape != xa.shape[:2] or st.shape[0] != xa.shape[0]:
        raise ValueError(f"token_merge_rows: x (B, N, C), start (B, rows + 1), members (B, N); got {xa.shape}, {st.shape}, {me.shape}")
    B, N, Cc = xa.shape
    y = np.empty((B, st.shape[1] - 1, Cc), np.float16)
    check(lib().tsd_token_merge_rows_f16(_ctx(ctx), xa.ctypes.data, B, N, Cc, st.shape[1] - 1, st.ctypes.data, me.ctypes.data, y.ctypes.data))
    return y


def token_unmerge_rows(y, row_of, ctx=None):
    """The unmerge launch alone (`tsd_token_unmerge_rows_f16`): y float16 (B, rows, C), row_of (B, N) -> (B, N, C)."""
    ya, ro = np.ascontiguousarray(y, dtype=np.float16), np.ascontiguousarray(row_of, dtype=np.int32)
    if ya.ndim != 3 or ro.ndim != 2 or ro.shape[0] != ya.shape[0]:
        raise ValueError(f"token_unmerge_rows: y (B, rows, C), row_of (B, N); got {ya.shape}, {ro.shape}")
    B, rows, Cc = ya.shape
    out = np.empty((B, ro.shape[1], Cc), np.float16)
    check(lib().tsd_token_unmerge_rows_f16(_ctx(ctx), ya.ctypes.data, B, ro.shape[1], Cc, rows, ro.ctypes.data, out.ctypes.data))
    return out
