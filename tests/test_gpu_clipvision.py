"""GPU: the CLIP vision encoder (model kind "clip_vision_h").  (1) its image front end, k_clip_image_patches, element-wise against the fp64
restatement under the derived bound of tests/clipvision_ref.py, through the guarded replay entry: every size at which the tables take
another shape (identity, 5 / 4 taps, upscaling with edge clamping on either axis, down-scaling with a crop on either axis, the smallest
and the largest side), on noise, a constant image and single-pixel impulses; pad columns, guards, batch position, run to run, refusals.
(2) the full-size encoder against the numpy restatement, and its bitwise properties.  (3) `generate(ip_image=, image_encoder=)`.

Measured on an MI355X (printed by the tests): see the docstrings of the tests.

Run as `python tests/test_gpu_clipvision.py jitter-child REPEATS` this file is the child of the jitter test: it prints one JSON line of
digests per case, computed with whatever library TSD_LIB names."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # the jitter child: the repository root (oracle) and the package before the reference modules load
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "stable-diffusion.mojo_amd")]

import clipvision_ref as R
import replay
from controlnet_ref import draw_params
from oracle import rng
from util import TOL_MODEL, rel_l2

pytestmark = pytest.mark.gpu
JITTER_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")
JITTER_REPEATS = 4
# (H, W, B): the largest at B = 1
SIZES = [(224, 224, 3), (225, 227, 3), (64, 96, 3), (96, 64, 3), (300, 500, 3), (512, 512, 3), (1024, 768, 3), (8, 8, 3), (2048, 2048, 1)]


@pytest.fixture(scope="module")
def ctx(gpu_ctx, tsd_mod):
    c = tsd_mod.Context(gpu_ctx.device)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def noise_image(H, W, seed):
    return np.random.default_rng(seed).uniform(0.0, 255.0, size=(3, H, W)).astype(np.float32)


def impulse_image(H, W):
    """Single pixels at 255 on a zero image: the four corners and two interior points, spread over the channels."""
    x = np.zeros((3, H, W), np.float32)
    for c, (y, xx) in enumerate([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 3), (H // 3, (2 * W) // 3)]):
        x[c % 3, y, xx] = 255.0
    return x


def batch_of(H, W, B):
    imgs = [noise_image(H, W, 31 * H + W), np.full((3, H, W), 255.0, np.float32), impulse_image(H, W)]
    if B == 1:   # the largest size: noise with the impulses' pixels forced to 255
        imgs = [np.maximum(imgs[0], imgs[2])]
    return np.stack(imgs[:B])


def check(name, images, out, info):
    """Every element inside the bound; the pad columns zero; no guard element changed.  Returns the worst error / bound ratio."""
    assert info["CHANGED"] == 0, f"{name}: {info['CHANGED']} guard elements written"
    assert (_bits(out[:, :, R.PATCH_K:]) == 0).all(), f"{name}: a pad column is not zero"
    worst = 0.0
    for b in range(images.shape[0]):
        ref, bnd = R.bound(images[b])
        err = np.abs(out[b, :, :R.PATCH_K].astype(np.float64) - ref)
        ratio = err / bnd
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio[i] <= 1.0, f"{name}: sample {b}, patch {i[0]}, column {i[1]}: |err| {err[i]:.3e} > bound {bnd[i]:.3e} (ref {ref[i]:.6f})"
        worst = max(worst, float(ratio[i]))
    return worst


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B", SIZES)
def test_kernel_matches_the_fp64_reference(ctx, H, W, B):
    """Worst error / bound over the nine sizes on an MI355X: printed per size (the fp16 half-ulp is most of the bound, so a worst case
    near 1 is a rounding at the half-ulp)."""
    images = batch_of(H, W, B)
    rc, out, info = R.run(ctx, images)
    assert rc == 0, replay.lib().tsd_last_error().decode()
    worst = check(f"{H}x{W}", images, out, info)
    _, ty, _, tx = R.tables(H, W)
    assert (info["TAPS_H"], info["TAPS_V"]) == (int(tx.max()), int(ty.max())), "the library's tables have other tap counts than the restatement's"
    assert info["LDS"] == 3 * info["ROWS"] * 14 * 4 and info["LDS"] < 32 * 1024
    print(f"[clipvision] {H}x{W} B={B}: taps {info['TAPS_H']}/{info['TAPS_V']}, {info['ROWS']} rows, {info['LDS']} B LDS, worst |err| / bound = {worst:.3f}")
    if (H, W) == (224, 224):   # the identity: the normalisation of the pixels themselves
        want = R.to_patches(R.normalise(images[0].astype(np.float64)))
        assert np.abs(out[0, :, :R.PATCH_K].astype(np.float64) - want).max() <= 2.0 ** -11 * np.abs(want).max() + 1e-6


def test_wider_pitch_zeroes_every_pad_column(ctx):
    images = batch_of(64, 96, 2)
    rc, out, info = R.run(ctx, images, ld=640)
    assert rc == 0 and out.shape == (2, 256, 640)
    check("ld 640", images, out, info)
    rc, base, _ = R.run(ctx, images)
    assert np.array_equal(_bits(out[:, :, :588]), _bits(base[:, :, :588]))


def test_batch_position_and_run_to_run_are_bitwise(ctx):
    H, W = 300, 500
    s, o1, o2 = noise_image(H, W, 5), noise_image(H, W, 6), impulse_image(H, W)
    rc, alone, _ = R.run(ctx, s[None])
    assert rc == 0
    for pos in range(3):
        others = [o1, o2]
        batch = np.stack(others[:pos] + [s] + others[pos:])
        rc, out, info = R.run(ctx, batch)
        assert rc == 0 and info["CHANGED"] == 0
        assert np.array_equal(_bits(out[pos]), _bits(alone[0])), f"the sample differs at position {pos} of B = 3"
        rc, again, _ = R.run(ctx, batch)
        assert np.array_equal(_bits(out), _bits(again)), "two runs differ"


def test_sides_outside_8_to_2048_are_refused(ctx, tsd_mod):
    E = tsd_mod._lib
    for H, W in ((7, 64), (64, 7), (2049, 224), (224, 2049)):
        rc, out, _ = R.run(ctx, np.zeros((1, 3, H, W), np.float32))
        assert rc == E.TSD_E_SHAPE, (H, W, rc)
        with pytest.raises(tsd_mod.TsdError) as e:
            tsd_mod.clip_image_patches(np.zeros((3, H, W), np.float32), ctx=ctx)
        assert e.value.code == E.TSD_E_SHAPE


def test_op_entry_agrees_with_the_replay_entry(ctx, tsd_mod):
    images = batch_of(96, 64, 3)
    rc, out, _ = R.run(ctx, images)
    got = tsd_mod.clip_image_patches(images, ctx=ctx)
    assert rc == 0 and got.shape == (3, 256, 592) and np.array_equal(_bits(got), _bits(out))
    assert np.array_equal(_bits(tsd_mod.clip_image_patches(images[1], ctx=ctx)), _bits(out[1]))


# ---- 2. the encoder ---------------------------------------------------------------------------------------------------------------------
SEED = 4242


class World:
    def __init__(self, tsd_mod):
        self.P = draw_params(tsd_mod.param_specs("clip_vision_h"), SEED)
        self.enc = tsd_mod.CLIPVision(params=self.P)
        self.sq = np.stack([noise_image(224, 224, 11), noise_image(224, 224, 12)])
        self.rect = noise_image(300, 500, 13)[None]
        self.ref = {}

    def reference(self, key, images):
        """Computed once per image set and left unchanged."""
        if key not in self.ref:
            self.ref[key] = [R.clip_vision_h(self.P, img, np.float32) for img in images]
        return self.ref[key]


@pytest.fixture(scope="module")
def world(gpu_ctx, tsd_mod):
    w = World(tsd_mod)
    yield w
    w.enc.model.close()


@pytest.mark.parametrize("which", ("square", "rect"))
def test_encoder_matches_the_numpy_restatement(world, which):
    """image_embeds and hidden_out at B = 2, 224x224 and at B = 1, 300x500 against the numpy restatement: relative L2 printed, TOL_MODEL."""
    images = world.sq if which == "square" else world.rect
    emb, hid = world.enc.forward(images, hidden=True)
    ref = world.reference(which, images)
    assert emb.shape == (len(images), 1024) and hid.shape == (len(images), 257, 1280) and np.isfinite(emb).all() and np.isfinite(hid).all()
    for b, (remb, rhid) in enumerate(ref):
        e1, e2 = rel_l2(emb[b], remb), rel_l2(hid[b], rhid)
        print(f"[clipvision] encoder {which} sample {b}: image_embeds rel_l2 {e1:.3e}, hidden rel_l2 {e2:.3e}")
        assert e1 <= TOL_MODEL and e2 <= TOL_MODEL


def test_encoder_bitwise_run_to_run_batch_position_and_hidden(world):
    imgs = np.stack([noise_image(64, 96, 21), noise_image(64, 96, 22), impulse_image(64, 96)])
    emb, hid = world.enc.forward(imgs, hidden=True)
    emb2, hid2 = world.enc.forward(imgs, hidden=True)
    assert np.array_equal(_bits(emb), _bits(emb2)) and np.array_equal(_bits(hid), _bits(hid2)), "two runs differ"
    plain = world.enc.forward(imgs)
    assert np.array_equal(_bits(plain), _bits(emb)), "image_embeds differ with hidden_out = NULL"
    for b in range(3):
        e1, h1 = world.enc.forward(imgs[b], hidden=True)
        assert np.array_equal(_bits(e1), _bits(emb[b])) and np.array_equal(_bits(h1), _bits(hid[b])), f"sample {b} alone differs from its row of B = 3"


def test_loaded_key_map_round_trip_gives_the_same_bits(world, tsd_mod):
    from tsd import checkpoint as ck
    twin = ck.load_clip_vision(ck.params_to_clip_vision(world.P))
    try:
        img = world.sq[:1]
        a, ha = world.enc.forward(img, hidden=True)
        b, hb = twin.forward(img, hidden=True)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(ha), _bits(hb))
    finally:
        twin.model.close()


def test_forward_refusals(world, tsd_mod, gpu_ctx):
    E = tsd_mod._lib
    lib = E.lib()
    from tsd._lib import f32, ptr
    img, emb = f32(np.zeros((1, 3, 32, 32))), f32(np.zeros((1, 1024)))
    ip = tsd_mod.IPAdapter(seed=1)
    try:
        assert lib.tsd_clip_vision_forward(ip.model.h, ptr(img), 1, 32, 32, ptr(emb), None) == E.TSD_E_ARG          # another kind
        assert lib.tsd_clip_vision_forward(None, ptr(img), 1, 32, 32, ptr(emb), None) == E.TSD_E_ARG
        assert lib.tsd_clip_vision_forward(world.enc.model.h, None, 1, 32, 32, ptr(emb), None) == E.TSD_E_ARG
        assert lib.tsd_clip_vision_forward(world.enc.model.h, ptr(img), 1, 32, 32, None, None) == E.TSD_E_ARG
        assert lib.tsd_clip_vision_forward(world.enc.model.h, ptr(img), 17, 32, 32, ptr(emb), None) == E.TSD_E_SHAPE
        assert lib.tsd_clip_vision_forward(world.enc.model.h, ptr(img), 1, 7, 32, ptr(emb), None) == E.TSD_E_SHAPE
        assert lib.tsd_model_context_width(world.enc.model.h) == E.TSD_E_ARG
        with pytest.raises(tsd_mod.TsdError) as e:
            world.enc.model.lora_add("layers.0.fc1.weight", np.zeros((5120, 2), np.float32), np.zeros((2, 1280), np.float32), 1.0)
        assert e.value.code == E.TSD_E_ARG
        with pytest.raises(ValueError):
            world.enc.forward(np.zeros((4, 32, 32), np.float32))
    finally:
        ip.model.close()


# ---- the jitter build -------------------------------------------------------------------------------------------------------------------
def jitter_cases(tsd, c, repeats):
    """[(name, [digest per repeat])]: the front end at three table shapes, and a forward of a seeded encoder."""
    out = []
    for H, W in ((64, 96), (300, 500), (1024, 768)):
        images = batch_of(H, W, 3)
        digs = []
        for _ in range(repeats):
            rc, y, info = R.run(c, images)
            assert rc == 0 and info["CHANGED"] == 0
            digs.append(hashlib.sha256(_bits(y).tobytes()).hexdigest()[:16])
        out.append((f"patches_{H}x{W}", digs))
    enc = tsd.CLIPVision(seed=77, ctx=c)
    imgs = batch_of(96, 64, 2)
    digs = []
    for _ in range(repeats):
        emb, hid = enc.forward(imgs, hidden=True)
        digs.append(hashlib.sha256(_bits(emb).tobytes() + _bits(hid).tobytes()).hexdigest()[:16])
    enc.model.close()
    out.append(("encoder_96x64", digs))
    return out


def test_jitter_build_reproduces_the_shipped_bits(tsd_mod, ctx):
    if not os.path.exists(JITTER_LIB):
        pytest.skip(f"{JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    here = jitter_cases(tsd_mod, ctx, 1)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "jitter-child", str(JITTER_REPEATS)], env=dict(os.environ, TSD_LIB=JITTER_LIB),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    there = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [r["name"] for r in there] == [n for n, _ in here]
    for (name, mine), theirs in zip(here, there):
        assert len(theirs["digests"]) == JITTER_REPEATS
        assert all(dg == mine[0] for dg in theirs["digests"]), f"{name}: the jitter build gave {len(set(theirs['digests']))} result(s), not the shipped bits"


# ---- 3. generate ------------------------------------------------------------------------------------------------------------------------
def test_generate_from_pixels_is_generate_from_the_encoders_embeds(world, tsd_mod, gpu_ctx):
    B, L, T = 2, 16, 77
    d = tsd_mod.Diffusion(seed=9, variant="diffusion_sd15")
    ip = tsd_mod.IPAdapter(seed=10)
    other = tsd_mod.Context(gpu_ctx.device)
    try:
        cx = rng.normal(7, 2101, B * T * 768).reshape(B, T, 768)
        uctx = rng.normal(7, 2102, B * T * 768).reshape(B, T, 768)
        img = np.stack([noise_image(64, 96, 41), noise_image(64, 96, 42)])
        kw = dict(uncond_context=uctx, cfg=True, cfg_scale=5.0, inference_steps=2, strength=1.0, L=L, return_latents=True, seeds=[901, 902])
        a = tsd_mod.generate(d, None, cx, ip_adapter=ip, ip_image=img, image_encoder=world.enc, **kw)
        b = tsd_mod.generate(d, None, cx, ip_adapter=ip, ip_image_embeds=world.enc.forward(img), **kw)
        plain = tsd_mod.generate(d, None, cx, **kw)
        assert a.shape == (B, 4, L, L) and np.isfinite(a).all()
        assert np.array_equal(_bits(a), _bits(b)), "generate(ip_image=) differs from generate(ip_image_embeds=enc.forward(image))"
        assert not np.array_equal(_bits(a), _bits(plain)), "the image prompt changed nothing"
        one = tsd_mod.generate(d, None, cx, ip_adapter=ip, ip_image=img[0], image_encoder=world.enc, **kw)   # one image for every sample
        assert np.array_equal(_bits(one[0]), _bits(a[0]))
        far = tsd_mod.CLIPVision(seed=3, ctx=other)
        try:
            with pytest.raises(ValueError, match="different contexts"):
                tsd_mod.generate(d, None, cx, ip_adapter=ip, ip_image=img, image_encoder=far, **kw)
        finally:
            far.model.close()
    finally:
        d.model.close(); ip.model.close(); other.close()


if __name__ == "__main__":
    assert sys.argv[1] == "jitter-child"
    import tsd
    tsd.set_strict(True)
    _c = tsd.Context(0)
    for _name, _digests in jitter_cases(tsd, _c, int(sys.argv[2])):
        print(json.dumps({"name": _name, "digests": _digests}), flush=True)
    _c.close()
