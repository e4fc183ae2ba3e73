"""Operands of shared self attention for its two test files: version-4 descriptors of tsd_debug_attn_run and, per sample, the ONE-sample
plain problem that states what it computes - its own S keys, or [own ; reference] as Sk = 2 S.  The rest is attn_ref's / attn64_ref's."""
import functools

import numpy as np

import attn64_ref as R
import attn_ref as A

#        d, forced kernel, H, table, S          (B = len(table); DIAG is 0 where S % 64 == 0: those are compared bit for bit)
CASES = [(40, 1, 3, (-1, 0, 0), 4), (40, 1, 2, (2, 2, -1), 72), (40, 2, 2, (-1, 0, -1, 2), 64), (40, 2, 1, (-1, 0, 0), 576),
         (64, 0, 3, (2, 2, -1), 72), (64, 0, 1, (-1, 0, 0), 576), (80, 0, 2, (-1, 0, -1, 2), 64), (80, 0, 3, (-1, 0, 0), 4),
         (160, 0, 1, (2, 2, -1), 576), (160, 0, 2, (-1, 0, 0), 72)]
IDS = [f"d{c[0]}k{c[1]}-h{c[2]}-{''.join('x' if t < 0 else str(t) for t in c[3])}-s{c[4]}" for c in CASES]


def gathered(d, ops, b, ref):
    """(descriptor, operands) of sample b alone: a plain launch over its own keys (ref < 0) or over [own ; sample ref's] keys."""
    H, hd, S = A.F(d, "H"), A.F(d, "D"), A.F(d, "SQ")
    q, k, v, _ = A.unpack_inputs(d, ops)
    ks = [b] if ref < 0 else [b, ref]
    g = A.attn_desc(1, H, hd, S, S * len(ks), kernel=A.F(d, "KERNEL"), diag=A.F(d, "DIAG"))
    g[A.AD["VERSION"]] = 2
    return g, A.pack(g, q[b:b + 1], np.concatenate([k[i:i + 1] for i in ks], axis=2), np.concatenate([v[i:i + 1] for i in ks], axis=2))


@functools.lru_cache(maxsize=None)
def case(i, kind="flat"):
    """(plain version-2 descriptor of the batch, version-4 descriptor, operands) - built once, shared, never modified."""
    hd, kern, H, table, S = CASES[i]
    base = A.attn_desc(len(table), H, hd, S, S, kernel=kern, diag=0 if S % 64 == 0 else 1)
    base[A.AD["VERSION"]] = 2
    ops = (R if hd == 64 else A).make_inputs(base, kind, seed=23)
    if kind == "spike":     # every sample's spike (its last key, 30 log2 units up at ITS queries) moves into its reference's keys: segment 1 only
        q, k, v, _ = (x.astype(np.float64) for x in A.unpack_inputs(base, ops))
        spikes = k[:, :, S - 1].copy()
        k[:, :, S - 1] = k[:, :, S - 2]
        for b, t in enumerate(table):
            if t >= 0:
                k[t, :, S - 1 - b] = spikes[b]
        ops = A.pack(base, q, k, v)
    d = np.concatenate([base, np.zeros(3, np.int64), [len(table)], np.array(table + (0,) * (8 - len(table)), np.int64)])      # WIN, GRID_H, GRID_W = 0
    d[A.AD["VERSION"]] = 4
    return base, d, ops
