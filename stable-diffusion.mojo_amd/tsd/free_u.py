"""FreeU (Si et al. 2023) on the full-size UNets: the 12-entry table of `tsd_model_set_freeu`, the two published ways of filling it, the
launch alone, and the scope `generate` / `generate_stream` set a table in.  No reference counterpart."""
import contextlib

import numpy as np

from ._lib import check, lib
from .utils import _ctx

FREEU_BLOCKS = 12
FREEU_CONSTANT, FREEU_MODULATED = 0, 1
# hidden width Ch of the twelve decoder residual blocks in pop order (the full-size step tables; tests hold it to oracle.spec)
FREEU_HIDDEN_WIDTHS = (1280, 1280, 1280, 1280, 1280, 1280, 1280, 640, 640, 640, 320, 320)
CONVENTIONS = ("diffusers", "channels")


def freeu_table(b1, b2, s1, s2, convention="diffusers"):
    """(b[12], s[12]) float32 for `Diffusion.set_freeu(table=...)` / `tsd_model_set_freeu`, block j = 0 .. 11 in pop order.

    "diffusers": (b1, s1) on j = 0, 1, 2 and (b2, s2) on j = 3, 4, 5 - diffusers' `enable_freeu`, which keys on the up block's
    `resolution_idx` 0 and 1 (three residual blocks each); ones elsewhere.
    "channels": (b1, s1) where the hidden tensor is 1280 wide (j = 0 .. 6) and (b2, s2) where it is 640 wide (j = 7, 8, 9), ones on
    j = 10, 11 - the authors' repository and the node UIs, which key on the hidden width.
    Both mappings are written from memory of those projects and could not be checked against them here; the library itself takes the
    12-entry table and depends on neither."""
    if convention not in CONVENTIONS:
        raise ValueError(f"freeu_table: convention {convention!r} ({', '.join(CONVENTIONS)})")
    b, s = np.ones(FREEU_BLOCKS, np.float32), np.ones(FREEU_BLOCKS, np.float32)
    if convention == "diffusers":
        first, second = range(0, 3), range(3, 6)
    else:
        first = [j for j, c in enumerate(FREEU_HIDDEN_WIDTHS) if c == 1280]
        second = [j for j, c in enumerate(FREEU_HIDDEN_WIDTHS) if c == 640]
    for j in first:
        b[j], s[j] = b1, s1
    for j in second:
        b[j], s[j] = b2, s2
    return b, s


def freeu_arguments(b1=None, b2=None, s1=None, s2=None, convention="diffusers", modulated=False, table=None):
    """The keywords of `Diffusion.set_freeu` as (b[12], s[12], mode)."""
    if table is not None:
        if any(v is not None for v in (b1, b2, s1, s2)):
            raise ValueError("set_freeu: pass table= or b1 / b2 / s1 / s2, not both")
        b, s = (np.ascontiguousarray(t, dtype=np.float32) for t in table)
        if b.shape != (FREEU_BLOCKS,) or s.shape != (FREEU_BLOCKS,):
            raise ValueError(f"set_freeu: table must be (b[{FREEU_BLOCKS}], s[{FREEU_BLOCKS}]), got {b.shape} and {s.shape}")
    else:
        if any(v is None for v in (b1, b2, s1, s2)):
            raise ValueError("set_freeu: b1, b2, s1 and s2 are all required (or table=)")
        b, s = freeu_table(b1, b2, s1, s2, convention)
    return b, s, FREEU_MODULATED if modulated else FREEU_CONSTANT


def freeu(h, r, b, s, mode=FREEU_CONSTANT, ctx=None):
    """The FreeU launch alone (`tsd_freeu_f16`): h float16 (B, H, W, Ch), r float16 (B, H, W, Cr) -> (h', r'): channels < Ch / 2 of h
    times b (mode 0) or times (b - 1) n + 1 with n the per-sample min-max normalised channel mean (mode 1); the four lowest spatial
    frequencies of every plane of r times s.  Either tensor may be None (it is skipped, and None comes back)."""
    ha = None if h is None else np.ascontiguousarray(h, dtype=np.float16)
    ra = None if r is None else np.ascontiguousarray(r, dtype=np.float16)
    if ha is None and ra is None:
        raise ValueError("freeu: h and r are both None")
    ref = ha if ha is not None else ra
    if ref.ndim != 4 or (ha is not None and ra is not None and ha.shape[:3] != ra.shape[:3]):
        raise ValueError("freeu: h (B, H, W, Ch) and r (B, H, W, Cr) must agree in B, H, W")
    B, H, W = ref.shape[:3]
    ho = None if ha is None else np.empty_like(ha)
    ro = None if ra is None else np.empty_like(ra)
    check(lib().tsd_freeu_f16(_ctx(ctx), None if ha is None else ha.ctypes.data, None if ra is None else ra.ctypes.data, B, H, W,
                              0 if ha is None else ha.shape[3], 0 if ra is None else ra.shape[3], float(b), float(s), int(mode),
                              None if ho is None else ho.ctypes.data, None if ro is None else ro.ctypes.data))
    return ho, ro


@contextlib.contextmanager
def freeu_scope(diffusion, freeu):
    """`generate(freeu=...)`: the dict's keywords are `Diffusion.set_freeu`'s; the model's previous table is back on every way out."""
    if freeu is None:
        yield
        return
    if not isinstance(freeu, dict):
        raise ValueError("freeu must be a dict of Diffusion.set_freeu's keywords (b1, b2, s1, s2, convention, modulated, table)")
    args = freeu_arguments(**freeu)
    prev = diffusion.freeu
    diffusion.set_freeu(table=args[:2], modulated=args[2] == FREEU_MODULATED)
    try:
        yield
    finally:
        if prev is None:
            diffusion.clear_freeu()
        else:
            diffusion.set_freeu(table=prev[:2], modulated=prev[2] == FREEU_MODULATED)
