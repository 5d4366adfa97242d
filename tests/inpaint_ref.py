"""Masked video-to-video, restated with torch on the CPU (not a test; tests/test_inpaint_host.py and tests/test_inpaint_gpu.py).

x0: the scaled clean latent of the clip (1,C,T,h,w) fp16; base: the job's seeded noise, same shape; m: the latent mask (T,h,w)
uint8, 1 = regenerate, 0 = keep; ts: the job's schedule.  The start is video-to-video's: add_noise(x0, base, ts[0]).  After the
scheduler step of ts[i] has produced z: where m == 1 z keeps its bits, where m == 0 z takes the bits of
known_i = add_noise(x0, base, ts[i+1]) = h16(h16(sa*x0) + h16(s1*base)), and of x0 itself after the last step.  Every operation
is a `torch.where` around fp16 tensor operations: a select, so nothing is multiplied by the mask."""
import torch


def add_noise_coefficients(scheduler, t: int, like):
    """(sqrt(a_t), sqrt(1 - a_t)) as `_SchedulerBase.add_noise` forms them: alphas_cumprod cast to the sample's dtype on the
    sample's device first, then fp16 tensor operations, then Python floats."""
    ac = scheduler.alphas_cumprod.to(device=like.device, dtype=like.dtype)
    return float(ac[t] ** 0.5), float((1 - ac[t]) ** 0.5)


def add_noise_ref(x0, noise, sa: float, s1: float):
    """fp16(fp16(sa * x0) + fp16(s1 * noise)): each product and the sum formed in fp32 and rounded to fp16 on its own."""
    a = (x0.float() * torch.tensor(sa, dtype=torch.float32)).half()
    b = (noise.float() * torch.tensor(s1, dtype=torch.float32)).half()
    return (a.float() + b.float()).half()


def renoise_ref(z, x0, base, m, sa, s1, last, s):
    """z (1,C,L,h,w) fp16 after a scheduler step -> the masked step's z; x0, base, m are the clip's, read at frames [s, s+L)."""
    L = z.shape[2]
    x = x0[:, :, s:s + L]
    known = x if last else add_noise_ref(x, base[:, :, s:s + L], sa, s1)
    return torch.where(m[s:s + L].bool()[None, None], z, known)


def paste_ref(z32, x0, m):
    return torch.where(m.bool()[None, None], z32, x0.float())


def latent_mask_ref(px, rule="nearest"):
    """Pixel mask (T,H,W), nonzero = regenerate -> (T,H/8,W/8) uint8 in {0,1}."""
    T, H, W = px.shape
    on = px != 0
    if rule == "nearest":
        return on[:, ::8, ::8].to(torch.uint8).contiguous()
    assert rule == "any"
    return on.view(T, H // 8, 8, W // 8, 8).any(dim=4).any(dim=2).to(torch.uint8)


def composite_ref(generated, original, mask):
    return torch.where((mask != 0)[..., None], generated, original)


def masked_job_ref(d, model, x0, base, m, co=False):
    """The masked job of the diffuser `d` (one rank), written out: a Python loop over the planner's windows that calls the public
    scheduler steps on the GPU and `renoise_ref` on the CPU -> (the final fp32 latent, the blend before the paste; None with
    `co`), on the CPU.  Windowed: one trajectory per window, the ramp blend, the paste.  `co`: one latent, the windows'
    predictions fused at every step (vdx/codenoise.py)."""
    from vdx import ops
    from vdx.codenoise import window_table
    unet, emb = model
    emb2 = torch.cat([emb[1:], emb[:1]], dim=0)
    cfg, sched, ts = d.cfg, d.scheduler, list(d.schedule)
    dev = x0.device
    x0c, basec, mc = x0.cpu(), base.cpu(), m.cpu()
    coef = [add_noise_coefficients(sched, t, x0) for t in ts[1:]] + [None]
    start = sched.add_noise(x0, base, ts[0])
    ctx = start.mean(dim=2, keepdim=True).contiguous() if cfg.use_ctx else None
    cp = d.plan()

    def renoise(z, i, s):
        sa, s1 = coef[i] if coef[i] is not None else (0.0, 0.0)
        return renoise_ref(z.cpu(), x0c, basec, mc, sa, s1, coef[i] is None, s).to(dev)

    if co:
        T = x0.shape[2]
        table = window_table(cp, T)
        slot = 2 * x0.shape[1] * cp.chunk * x0.shape[3] * x0.shape[4]
        rows, wn = table.rows(1, cp.per_rank, slot), table.wn.to(dev)
        local = torch.zeros((cp.per_rank, slot), dtype=torch.float16, device=dev)
        z = start.clone()
        sched.reset()
        for i, t in enumerate(ts):
            for j, (s, e) in enumerate(cp.for_rank(0)):
                x = ops.cfg_input(z[:, :, s:e].contiguous(), ctx, cfg.context_weight)
                noise = unet(x, t, encoder_hidden_states=emb2).sample
                local[j, :noise.numel()].copy_(noise.reshape(-1))
            z = renoise(sched.step_cfg_windows(local, rows, wn, t, z, cfg.guidance_scale), i, 0)
        return z.float().cpu(), None
    chunks = []
    for s, e in cp.for_rank(0):
        lat = start[:, :, s:e].clone()
        sched.reset()
        for i, t in enumerate(ts):
            noise = unet(ops.cfg_input(lat, ctx, cfg.context_weight), t, encoder_hidden_states=emb2).sample
            lat = renoise(sched.step_cfg(noise, t, lat, cfg.guidance_scale), i, s)
        chunks.append((s, e, lat))
    blended = d.blend(chunks, start, cp.overlap).cpu()
    return paste_ref(blended, x0c, mc), blended
