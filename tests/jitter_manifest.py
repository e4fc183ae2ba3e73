"""One manifest of replay cases for the -DTSD_JITTER build (`make jitter`, csrc/lds_dma.h: tsd_jitter() - a random wave-level delay where
waves meet), and the child process that runs it (test infrastructure; importing it needs no GPU).

The fp64 tests (test_gpu_gemm_ref.py, test_gpu_attn_ref.py, test_gpu_chain_ref.py, test_gpu_norm_ref.py, test_gpu_elem_ref.py,
test_gpu_lora.py) hold the SHIPPED library's result of every case below to an fp64 reference: they catch a kernel that is wrong every time.
A kernel that is wrong only when its waves drift apart gives, under the jitter build, other bits than the shipped library on the same
operands - so tests/test_gpu_jitter_replay.py runs every case once on the shipped library in its own process, REPEATS times on the jitter
library in a child (this file as a program), and compares digests.  The cases are built from the tables those tests use, with their seeds.

A case is (family, name, entry, desc, extra, recipe, ctx_opt):
    family   gemm | attn | chain | norm | elem | lora | model
    name     unique over the whole manifest
    entry    the replay entry of include/tsd.h (or, for the model family, the host call)
    desc     the int64 descriptor (lora: the shape tuple of test_gpu_lora.py; model: the shape of the call)
    extra    gemm: the forced tile configuration (-1: the dispatcher's choice); otherwise None
    recipe   how the operands are made: (maker, arguments...) - see _operands
    ctx_opt  None, or (variable, value): the case runs on a context created with that option in the environment

A digest is the sha1 of the family name, the bytes of every output slot as the entry returned it (pitch gaps and their fill included), and
the info fields the family's fp64 test asserts (INFO_FIELDS) as little-endian int64.  No wall-clock or tick value enters it.

    python tests/jitter_manifest.py FAMILY [REPEATS] [I/N]
runs the cases of FAMILY (the I-th of N interleaved slices) REPEATS times each on the library TSD_LIB names (default: the shipped one) and
prints one JSON line per case: {"name", "status", "digests": [REPEATS hex strings]}.  FAMILY `selftest` prints the number of distinct words
REPEATS (<= 64) launches of the jitter build's hazard-on-purpose kernel stored (tsd_debug_jitter_selftest)."""
import collections
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "stable-diffusion.mojo_amd")
for _p in (ROOT, PKG, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import attn_ref as A  # noqa: E402
import chain_ref as R  # noqa: E402
import elem_ref as E  # noqa: E402
import gemm_ref as G  # noqa: E402
import lora_ref  # noqa: E402
import norm_ref as N  # noqa: E402
import replay  # noqa: E402

Case = collections.namedtuple("Case", "family name entry desc extra recipe ctx_opt")
FAMILIES = ("gemm", "attn", "chain", "norm", "elem", "lora", "model")
JITTER_LIB = os.path.join(PKG, "lib", "libtsd_jitter.so")
SK256 = ("TSD_GEMM_SK256", "3")
MODEL_SEED = 1234

# the info fields of each entry that enter the digest: what the family's fp64 test asserts today
INFO_FIELDS = {
    "gemm": (0, 1, 2),                                                       # cfg, split-K ways, guard / pitch-gap writes
    "attn": tuple(A.AI[k] for k in ("KERNEL", "EXACT_WGS", "DIAG", "XCD_MAP", "CHANGED")),
    "chain": tuple(R.CI[k] for k in ("CHANGED", "RAN")),
    "norm": tuple(N.NI[k] for k in ("CHANGED", "NSLAB", "OWN_PASS", "PREREDUCE", "FINALIZE", "COMPOSITE")),
    "elem": tuple(E.EI[k] for k in ("NB", "PASSES", "NONFINITE", "CHANGED")),
    "lora": (),
    "model": (),
}

# Kernels that carry at least one tsd_jitter() point: (listing stem, kernel name).  tests/test_jitter_manifest_cpu.py finds the point (a clock
# read and an s_sleep the shipped listing does not have) in every instantiation of each in csrc/build_jitter/, and neither in csrc/build/:
# each family above runs a perturbed kernel, and a kernel added here without a point fails on the CPU.
JITTER_KERNELS = (
    ("kernels_gemm", "gemm_kernel"),
    ("kernels_attn", "flash_attn_kernel"), ("kernels_attn8", "flash_attn8_kernel"),
    ("kernels_chain", "attn_chain_kernel"),
    ("kernels_guidance", "k_cfg_moments"),
    ("kernels_norm", "k_gn_partial"), ("kernels_norm", "k_gn_prereduce"), ("kernels_norm", "k_gn_apply"),
    ("kernels_elementwise", "k_softmax_rows"), ("kernels_elementwise", "k_softmax_rows_h8"), ("kernels_elementwise", "k_small_linear"),
    ("kernels_lora", "k_lora_merge"),
)
# gemm_kernel sleeps in the shipped build too: the bounded wait of its split-K hand-off (kernels_gemm.hip) is an s_sleep loop of its own
SHIPPED_SLEEPS = ("gemm_kernel",)


def _lora_tables():
    """(general-operand shapes (O, I, r, s), EXACT_CASES) of test_gpu_lora.py - read from that module, so the two cannot drift."""
    import test_gpu_lora as T
    general = T.test_merge_of_general_operands_stays_inside_the_fp32_interval.pytestmark[0].args[1]
    return [tuple(c) for c in general], [tuple(c) for c in T.EXACT_CASES]


# ---- the manifest ------------------------------------------------------------------------------------------------------------------
def _gemm():
    out = []
    for name, d, cfgs in G._sweep_cases():
        for cfg in cfgs:
            if cfg == 30 and int(d[G.GD["N"]]) % 160:   # (the fp64 sweep skips the 160-wide halo tile on a 128-wide shape)
                continue
            out.append(Case("gemm", f"gemm/{name}/cfg{cfg}", "tsd_debug_gemm_run", d, cfg, ("gemm", cfg), None))
    for name, d, _ in G.SPLITS:
        out.append(Case("gemm", f"gemm/split/{name}", "tsd_debug_gemm_run", d, -1, ("gemm", 3), None))
    out.append(Case("gemm", "gemm/vt_tail", "tsd_debug_gemm_run", G._vt_desc(), -1, ("gemm", 5), None))
    d = G.dense_desc(M=1024, N=1280, K=5120, epi=G.EPI["BIAS_N"] | G.EPI["RESIDUAL"], rps_hint=256)
    out.append(Case("gemm", "gemm/optin_256_row_split", "tsd_debug_gemm_run", d, -1, ("gemm", 4), SK256))
    return out


def _attn():
    out = [Case("attn", f"attn/{name}", "tsd_debug_attn_run", d, None, ("attn", kind, 7), None) for name, d, kind in A.sweep()]
    out += [Case("attn", f"attn/softmax/{name}", "tsd_debug_attn_run", d, None, ("softmax", 5), None) for name, d in A.softmax_sweep()]
    return out


def _chain():
    return [Case("chain", f"chain/{name}", "tsd_debug_chain_run", d, None, ("chain", kind, R.SEED), None) for name, d, kind in R.SWEEP]


def _norm():
    out = [Case("norm", f"norm/gn/{name}", "tsd_debug_norm_run", d, None, ("norm", 11, sr), None) for name, d, sr, _ in N.sweep()]
    out += [Case("norm", f"norm/{name}", "tsd_debug_norm_run", d, None, ("norm", 12, 32), None) for name, d in N.ln_sweep()]
    return out


def _elem():
    return [Case("elem", f"elem/{name}", "tsd_debug_elem_run", d, None, ("elem", 11, kind), None)
            for name, d, kind, _ in E.sweep() if E.mode_of(d) == "SMALL_LINEAR"]


def _lora():
    general, exact = _lora_tables()
    out = [Case("lora", "lora/general/O%d_I%d_r%d" % c[:3], "tsd_lora_merge_f32", c, None, ("lora_general",), None) for c in general]
    out += [Case("lora", "lora/exact/O%d_I%d_k%d_r%d_il%d_rows%d+%d" % (c[0], c[1], c[2], c[3], c[5], c[6], c[7]), "tsd_lora_merge_f32", c,
                 None, ("lora_exact",), None) for c in exact]
    return out


def _model():
    """The product's own graphs outside the headline shape (B = 8, L = 64 without CFG is test_jitter_build_reproduces_the_shipped_bits)."""
    return [Case("model", "model/unet_cfg_b2_l16", "Session.step", (2, 16, 1), None, ("unet",), None),
            Case("model", "model/unet_b3_l24", "Session.step", (3, 24, 0), None, ("unet",), None),
            Case("model", "model/decoder_l16", "Decoder.forward", (1, 16), None, ("decoder",), None),
            Case("model", "model/encoder_128px", "Encoder.forward", (1, 128), None, ("encoder",), None),
            Case("model", "model/clip_b2", "CLIP.forward", (2, 77), None, ("clip",), None)]


_BUILD = dict(gemm=_gemm, attn=_attn, chain=_chain, norm=_norm, elem=_elem, lora=_lora, model=_model)
_CACHE = {}


def family(name):
    if name not in _CACHE:
        _CACHE[name] = _BUILD[name]()
    return _CACHE[name]


def manifest():
    """Every case, in order."""
    return [c for f in FAMILIES for c in family(f)]


def select(fam, part=None):
    """The cases of a family; part (i, n): the i-th of n interleaved slices (every n-th case from i on)."""
    cases = family(fam)
    return cases if part is None else cases[part[0]::part[1]]


# ---- digests -----------------------------------------------------------------------------------------------------------------------
def digest(fam, outs, info=()):
    """sha1 over the family name, every output array's bytes in slot order, and the selected info fields as little-endian int64."""
    h = hashlib.sha1(fam.encode())
    for o in outs:
        h.update(np.ascontiguousarray(o).tobytes())
    h.update(np.asarray([int(v) for v in info], "<i8").tobytes())
    return h.hexdigest()


def info_of(fam, info):
    return [int(info[i]) for i in INFO_FIELDS[fam]]


# ---- running a case ------------------------------------------------------------------------------------------------------------------
def _operands(case):
    r = case.recipe
    if r[0] == "gemm":
        return G.make_operands(case.desc, r[1])
    if r[0] == "attn":
        return A.make_inputs(case.desc, r[1], seed=r[2])
    if r[0] == "softmax":
        return {"X": A.softmax_inputs(case.desc, seed=r[1])}
    if r[0] == "chain":
        return R.make_inputs(case.desc, r[1], seed=r[2])
    if r[0] == "norm":
        return N.make_inputs(case.desc, seed=r[1], slab_rows=r[2])
    if r[0] == "elem":
        return E.make_inputs(case.desc, r[1], r[2])
    if r[0] == "lora_general":
        O, I, rank, s = case.desc
        return lora_ref.general_operands(O, I, O, rank, seed=O) + (s, 0, 0, 0)
    if r[0] == "lora_exact":
        O, I, k, rank, s, inter, row0, rows = case.desc
        cols = I * (k * k if k else 1)
        W, up, down = lora_ref.exact_operands(O, cols, rows, rank, seed=O * 131 + I)
        return (W.reshape(O, I, k, k) if k else W, up, down, s, k, inter, row0)
    rng = np.random.default_rng(MODEL_SEED)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    if r[0] == "unet":
        B, L, cfg = case.desc
        return dict(lat=f32(B, 4, L, L), cond=f32(B, 77, 768), uncond=f32(B, 77, 768) if cfg else None)
    if r[0] == "decoder":
        return dict(x=f32(case.desc[0], 4, case.desc[1], case.desc[1]))
    if r[0] == "encoder":
        B, S = case.desc
        return dict(x=rng.uniform(-1, 1, (B, 3, S, S)).astype(np.float32), noise=f32(B, 4, S // 8, S // 8))
    return dict(tokens=rng.integers(0, 49408, case.desc).astype(np.int32))


_REPLAY = {
    "gemm": lambda c: (G.GO, G.INPUTS, G.OUTPUTS, G.dtype_of, G.extents, (c.extra,)),
    "attn": lambda c: (A.AO, A.INPUTS, ("O",), A.dtype_of, A.extents, ()),
    "chain": lambda c: (R.CO, R.INPUTS, R.OUTPUTS, R.dtype_of, R.extents, ()),
    "norm": lambda c: (N.NO, N.INPUTS, N.OUTPUTS, N.dtype_of, N.extents, ()),
    "elem": lambda c: (E.EO, E.INPUTS, E.OUTPUTS, E.dtype_of, E.extents, ()),
}


class _Models:
    """The four random-init models of the model family, created when a case first asks and closed with the runner."""

    def __init__(self, tsd, ctx):
        self.tsd, self.ctx, self.m = tsd, ctx, {}

    def get(self, kind):
        if kind not in self.m:
            cls = dict(unet=self.tsd.Diffusion, decoder=self.tsd.Decoder, encoder=self.tsd.Encoder, clip=self.tsd.CLIP)[kind]
            self.m[kind] = cls(seed=MODEL_SEED, ctx=self.ctx)
        return self.m[kind]

    def close(self):
        for m in self.m.values():
            m.model.close()


def _run_model(tsd, models, case, ops):
    kind = case.recipe[0]
    m = models.get(kind)
    if kind == "unet":
        B, L, cfg = case.desc
        s = tsd.Session(m.model, None, B, L, 77, cfg=bool(cfg))
        try:
            s.set_schedule(1000, 2, 0)
            s.upload(ops["lat"], ops["cond"], ops["uncond"], None, cfg_scale=7.5)
            s.step(0)
            return s.latents()
        finally:
            s.close()
    if kind == "decoder":
        return m.forward(ops["x"])
    if kind == "encoder":
        return m.forward(ops["x"], ops["noise"])
    return m.forward(ops["tokens"])


def run_once(tsd, ctx, case, ops, models=None):
    """One run of a case on the loaded library: (status, digest)."""
    if case.family == "model":
        return 0, digest("model", [_run_model(tsd, models, case, ops)])
    if case.family == "lora":
        W, up, down, s, k, inter, row0 = ops
        rc, out = lora_ref.merge_op(tsd, ctx, W, up, down, s, k=k, interleave=inter, row0=row0)
        return rc, digest("lora", [out])
    slots, inputs, outputs, dtype_of, extents, extra = _REPLAY[case.family](case)
    rc, outs, info = replay.run(case.entry, ctx, case.desc, ops, slots, inputs, outputs, dtype_of, extents, extra=extra)
    return rc, digest(case.family, [outs[s] for s in outputs if s in outs], info_of(case.family, info))


def run_cases(tsd, cases, repeats=1, emit=None, device=0):
    """Every case `repeats` times on the library this process loaded, one context per context option: [{name, status, digests}].
    emit, when given, receives each record as soon as its case is done."""
    ctxs, out = {}, []
    models = None
    try:
        for case in cases:
            if case.ctx_opt not in ctxs:
                if case.ctx_opt:     # read once, by tsd_ctx_create; the environment is restored at once
                    os.environ[case.ctx_opt[0]] = case.ctx_opt[1]
                try:
                    ctxs[case.ctx_opt] = tsd.Context(device)
                finally:
                    if case.ctx_opt:
                        del os.environ[case.ctx_opt[0]]
            ctx = ctxs[case.ctx_opt]
            if case.family == "model" and models is None:
                models = _Models(tsd, ctx)
            ops = _operands(case)
            runs = [run_once(tsd, ctx, case, ops, models) for _ in range(repeats)]
            status = sorted({rc for rc, _ in runs})
            rec = dict(name=case.name, status=status[0] if len(status) == 1 else status, digests=[dg for _, dg in runs])
            out.append(rec)
            if emit:
                emit(rec)
    finally:
        if models:
            models.close()
        for c in ctxs.values():
            c.close()
    return out


def selftest(tsd, n=64, device=0):
    """tsd_debug_jitter_selftest on the loaded library: the distinct count (>= 1), or the negative status and its message."""
    ctx = tsd.Context(device)
    try:
        rc = tsd._lib.lib().tsd_debug_jitter_selftest(ctx.h, int(n))
        return rc, (tsd._lib.last_error() if rc < 0 else "")
    finally:
        ctx.close()


# ---- the listings: where the jitter points are ----------------------------------------------------------------------------------------
_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")


def points_per_function(listing):
    """{function symbol: (s_sleep instructions, s_memtime instructions)} of one compiler listing
    (csrc/build*/<file>-hip-amdgcn-amd-amdhsa-gfx950.s).  tsd_jitter() reads the clock (s_memtime) and sleeps on its low bits."""
    types, func, out = set(), None, {}
    with open(listing) as f:
        for ln in f:
            s = ln.strip()
            if s.startswith(".type") and "@function" in s:
                types.add(s.split()[1].split(",")[0])
                continue
            m = _LABEL.match(ln)
            if m:
                if func is None and m.group(1) in types:
                    func = m.group(1)
                    out[func] = (0, 0)
                elif func is not None and m.group(1).startswith(".Lfunc_end"):
                    func = None
                continue
            if func is not None:
                mn = s.split(";")[0].split()[:1]
                if mn == ["s_sleep"]:
                    out[func] = (out[func][0] + 1, out[func][1])
                elif mn == ["s_memtime"]:
                    out[func] = (out[func][0], out[func][1] + 1)
    return out


def kernel_of(symbol):
    """The function name of an Itanium-mangled symbol (_Z<len><name>...), or the symbol itself."""
    m = re.match(r"_Z(\d+)", symbol)
    return symbol[m.end():m.end() + int(m.group(1))] if m else symbol


def listing(build_dir, stem, arch="gfx950"):
    return os.path.join(PKG, "csrc", build_dir, f"{stem}-hip-amdgcn-amd-amdhsa-{arch}.s")


# ---- the child ----------------------------------------------------------------------------------------------------------------------
def main(argv):
    fam = argv[1]
    repeats = int(argv[2]) if len(argv) > 2 else 8
    part = tuple(int(x) for x in argv[3].split("/")) if len(argv) > 3 else None
    import tsd
    tsd.set_strict(True)

    def emit(rec):
        print(json.dumps(rec), flush=True)

    if fam == "selftest":
        rc, msg = selftest(tsd, repeats)
        emit(dict(name="jitter_selftest", status=min(rc, 0), digests=[], distinct=max(rc, 0), message=msg))
        return 0
    run_cases(tsd, select(fam, part), repeats, emit=emit)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
