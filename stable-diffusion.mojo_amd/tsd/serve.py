"""tsd.serve - host-side continuous batching over a slot session (no reference counterpart: pipeline.mojo denoises one prompt at a time).

A `Session` in slot mode (`Session.slots_open`) gives every sample of its batch its own request, schedule index and guidance scale; one
`advance()` is one UNet forward for all of them.  `SlotScheduler` keeps the slots full from an iterator of requests: before every advance
each free slot takes the next request, a slot that finishes yields its latents and is free again.  A request that arrives while the
others are at step 3 of 50 starts at once; img2img requests of different strength - different start indices - share the batch.

The scheduler only calls the slot methods (`B`, `LH` / `LW` or else `L`, `num_steps`, `slot_start`, `slot_set_inpaint`, `advance`, `slot_latents` - and
`slot_set_guidance_rescale` for a request that asks for it), so it runs against any object that has them (tests/test_slots_cpu.py and
tests/test_slot_inpaint_cpu.py drive it without a GPU).
"""
from collections import namedtuple

import numpy as np

from ._lib import check_guidance_rescale, latent_shape

# One request.  latents None: txt2img from `seed`.  latents (4,L,L) with strength s in [0,1]: img2img by the rule of `generate`
# (sampler.mojo:68-70) - the first n - int(n * s) steps are skipped and the latents are noised to that timestep from `seed`.
# mask: inpainting - `latents` are the known latents and the mask says where to regenerate (1) and where to keep them (0): a latent mask
# (LH,LW) / (1,LH,LW) is used as given, a pixel mask (8LH,8LW) / (1,8LH,8LW) goes through `tsd.utils.latent_mask` with `mask_mode`.
# LH, LW are the session's sides (`session_shape`): its `LH` / `LW`, or its `L` twice for a session object that has only that.
_RequestFields = namedtuple("Request", "id context uncond seed cfg_scale latents strength mask mask_mode")
_RequestFields.__new__.__defaults__ = (None, 0, 7.5, None, None, None, "any")


class Request(_RequestFields):
    """The nine positional fields above - the tuple a queue may hold in place of a Request - and, by keyword only, guidance_rescale in
    [0, 1]: the request's guidance rescale (`Session.slot_set_guidance_rescale`), per request like cfg_scale; 0 = off.  The keyword is
    an attribute beside the tuple: `_fields`, unpacking and comparison stay those of the nine fields; `_replace` keeps it."""
    guidance_rescale = 0.0   # for an instance made without __new__ (`_make`)

    def __new__(cls, *fields, guidance_rescale=0.0, **kw):
        self = super().__new__(cls, *fields, **kw)
        self.guidance_rescale = check_guidance_rescale(guidance_rescale)   # ValueError outside [0, 1]; CFG is the session's to check
        return self

    def _replace(self, **kw):
        phi = kw.pop("guidance_rescale", self.guidance_rescale)
        r = super()._replace(**kw)
        r.guidance_rescale = phi
        return r


def session_shape(session):
    """(LH, LW) of a session: its `LH` / `LW` attributes, or `L` (an int or a pair) for an object that has only that."""
    if hasattr(session, "LH") and hasattr(session, "LW"):
        return int(session.LH), int(session.LW)
    return latent_shape(session.L)


def request_latent_mask(r, session):
    """The latent mask (LH,LW) float32 of request r for `session` (its shape, its context for a pixel mask), or None without a mask.
    ValueError for a mask without latents or of another shape."""
    if r.mask is None:
        return None
    if r.latents is None:
        raise ValueError(f"request {r.id!r}: a mask needs `latents`, the known latents it keeps")
    (LH, LW), ctx = session_shape(session), getattr(session, "ctx", None)
    m = np.ascontiguousarray(r.mask, dtype=np.float32)
    if m.ndim == 3 and m.shape[0] == 1:
        m = m[0]
    if m.shape == (LH, LW):
        return np.ascontiguousarray(m)
    if m.shape == (8 * LH, 8 * LW):
        from . import utils
        return np.ascontiguousarray(utils.latent_mask(m[None], r.mask_mode, ctx=ctx)[0])
    raise ValueError(f"request {r.id!r}: mask must have shape {(LH, LW)} or {(8 * LH, 8 * LW)} (with or without a leading 1), got {np.shape(r.mask)}")


def start_index(num_steps, strength):
    """`generate`'s img2img rule: the schedule index a request of this strength starts at (None: 0, the whole schedule)."""
    if strength is None:
        return 0
    if not (0.0 <= strength <= 1.0):
        raise ValueError(f"strength must be between 0 and 1, got {strength}")
    return num_steps - int(num_steps * strength)


class SlotScheduler:
    """Iterate to run: yields (id, latents (4,L,L)) as slots finish, in slot order within one advance.

    Greedy filling: before each advance every free slot takes the next request of the queue, so no advance runs with a free slot while
    a request waits.  `advances`, `active_ticks` and `occupancy` (active slot-ticks over B * advances) describe the run so far.
    A request whose strength leaves no step (start index == num_steps) is yielded as given, without taking a slot."""

    def __init__(self, session, requests):
        self.session, self.requests = session, iter(requests)
        self.B, self.n = session.B, session.num_steps
        self.owner = [None] * self.B  # request id per slot, None = free
        self.advances = 0
        self.active_ticks = 0
        self._exhausted = False

    @property
    def occupancy(self):
        return self.active_ticks / (self.B * self.advances) if self.advances else 0.0

    def _fill(self):
        """Start queued requests in the free slots; returns the requests that need no step at all."""
        passed = []
        for b in range(self.B):
            while self.owner[b] is None and not self._exhausted:
                try:
                    r = next(self.requests)
                except StopIteration:
                    self._exhausted = True
                    break
                if not isinstance(r, Request):
                    r = Request(*r)
                # a request that cannot run raises here, before its slot (or any other) is touched
                mask = request_latent_mask(r, self.session)
                phi = check_guidance_rescale(r.guidance_rescale, getattr(self.session, "cfg", True))
                i0 = start_index(self.n, r.strength if r.latents is not None else None)
                if i0 >= self.n:  # strength 0: the image as it is
                    passed.append((r.id, np.asarray(r.latents, dtype=np.float32)))
                    continue
                self.session.slot_start(b, r.context, r.uncond, latents=r.latents, noise_at_start=r.latents is not None, seed=r.seed,
                                        start_index=i0, cfg_scale=r.cfg_scale)
                if mask is not None:
                    self.session.slot_set_inpaint(b, mask, r.latents)
                if phi > 0.0:
                    self.session.slot_set_guidance_rescale(b, phi)
                self.owner[b] = r.id
        return passed

    def __iter__(self):
        while True:
            for item in self._fill():
                yield item
            busy = sum(o is not None for o in self.owner)
            if not busy:
                return
            finished = self.session.advance()
            self.advances += 1
            self.active_ticks += busy
            for b in finished:
                rid, self.owner[b] = self.owner[b], None
                yield rid, self.session.slot_latents(b)


def generate_stream(diffusion, decoder, requests, B, L, T=77, cfg=True, inference_steps=50, num_training_steps=1000, sampler="ddpm",
                    eta=0.0, spacing="leading", return_latents=False, stats=None, prediction="epsilon", zero_terminal_snr=False, controlnet=None,
                    control_image=None, freeu=None, **control_keywords):
    """Continuous batching of `generate`: `requests` is an iterator of `Request`s (or tuples in its field order); yields (id, image
    (3,8LH,8LW) in [0,255]) - or (id, latents) with return_latents or without a decoder - as requests finish, B at a time on the device.
    L is the latent side or a pair (LH, LW): one shape for the whole stream.
    A txt2img request gives what `generate(..., seeds=[...])` gives for it in the same sample position.  An img2img request indexes the
    FULL timestep list (its step i draws stream 16 + i of its seed), where `generate` drops the skipped entries and counts from 0.
    A request with a `mask` is inpainted in its slot (`Session.slot_set_inpaint`) next to the others: no drain, no extra launch.
    A request with `guidance_rescale` > 0 is rescaled in its slot (`Session.slot_set_guidance_rescale`), as `generate(...,
    guidance_rescale=...)` rescales it; it needs cfg=True.
    prediction / zero_terminal_snr are `generate`'s keywords (`Session.set_prediction`): they belong to the model, so to the whole stream,
    never to a request.
    Finished latents are decoded through `decoder.forward`, one image per call.  `stats`, a dict, receives advances / active_ticks / occupancy when the stream ends.
    controlnet / control_image (and generate's other control_* keywords) are refused: the stream runs on a slot session, and per-slot
    control is not supported (`generate` runs lockstep sessions and takes them).  generate's ip_adapter / ip_image_embeds / ip_scale /
    ip_start / ip_end / ip_image / ip_hidden / ip_uncond_hidden are refused for the same reason: per-slot adapters are not supported.
    freeu is `generate`'s keyword: FreeU is state of the model, so of the whole stream; the model's previous table is back when the stream
    ends, however it ends."""
    if any(k.startswith("ip_") for k in control_keywords):
        raise ValueError("generate_stream runs on a slot session, which has no IP-Adapter (per-slot adapters are not supported); use generate()")
    if controlnet is not None or control_image is not None or control_keywords:
        raise ValueError("generate_stream runs on a slot session, which has no ControlNet (per-slot control is not supported); use generate()")
    from .free_u import freeu_scope
    from .model import Session
    from .utils import _unary
    with freeu_scope(diffusion, freeu):
        yield from _stream(diffusion, decoder, requests, B, L, T, cfg, inference_steps, num_training_steps, sampler, eta, spacing, return_latents,
                           stats, prediction, zero_terminal_snr, Session, _unary)


def _stream(diffusion, decoder, requests, B, L, T, cfg, inference_steps, num_training_steps, sampler, eta, spacing, return_latents, stats,
            prediction, zero_terminal_snr, Session, _unary):
    sess = Session(diffusion.model, None, B, L, T, cfg=cfg)
    try:
        if (prediction, bool(zero_terminal_snr)) != ("epsilon", False):
            sess.set_prediction(prediction, zero_terminal_snr)
        if (sampler, eta, spacing) != ("ddpm", 0.0, "leading"):
            sess.set_sampler(sampler, eta, spacing)
        sess.set_schedule(num_training_steps, inference_steps, 0)
        sess.slots_open()
        sched = SlotScheduler(sess, requests)
        for rid, lat in sched:
            if decoder is None or return_latents:
                yield rid, lat
            else:
                yield rid, _unary("tsd_rescale_images_f32", decoder.forward(lat), diffusion.model.ctx)  # pipeline.mojo:127
        if stats is not None:
            stats.update(advances=sched.advances, active_ticks=sched.active_ticks, occupancy=sched.occupancy)
    finally:
        sess.close()
