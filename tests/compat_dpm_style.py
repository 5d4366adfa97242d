"""Driver for tests/test_dpm_gpu.py, run as `python -m vdx.compat.run tests/compat_dpm_style.py`.

The scheduler swap of Zeroscope's published recipe, as a user's script writes it against diffusers —
`pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)` — followed by the stock CFG loop on
`pipe.scheduler.timesteps` / `.step(...).prev_sample`, twice (a second `set_timesteps` starts a new trajectory)."""
import torch
from diffusers import DiffusionPipeline, DPMSolverMultistepScheduler      # -> vdx.compat.diffusers_shim


def main():
    device = "cuda"
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    ddim = pipe.scheduler
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    assert type(pipe.scheduler).__name__ == "DPMSolverMultistepScheduler" and pipe.scheduler is not ddim
    pipe.to(device)
    toks = pipe.tokenizer(["a panda", ""], padding="max_length", max_length=pipe.tokenizer.model_max_length, truncation=True,
                          return_tensors="pt")
    with torch.no_grad():
        emb = pipe.text_encoder(toks.input_ids.to(device))[0]
    cond, uncond = emb[:1], emb[1:]
    torch.manual_seed(0)
    base = torch.randn(1, pipe.unet.config.in_channels, 4, 16, 32, device=device, dtype=torch.float16)
    base = base * pipe.scheduler.init_noise_sigma

    def denoise(lat, steps):
        pipe.scheduler.set_timesteps(steps, device=device)
        for t in pipe.scheduler.timesteps:
            x = pipe.scheduler.scale_model_input(torch.cat([lat] * 2), t)
            with torch.no_grad():
                noise = pipe.unet(x, t, encoder_hidden_states=torch.cat([uncond, cond])).sample
            u, c = noise.chunk(2)
            lat = pipe.scheduler.step(u + 7.5 * (c - u), t, lat).prev_sample
        return lat

    a, b = denoise(base.clone(), 4), denoise(base.clone(), 4)
    assert a.shape == base.shape and bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)
    print(f"COMPAT-DPM-OK steps 4 timesteps {pipe.scheduler._host_timesteps} |lat| {float(a.float().abs().mean()):.4f}")


if __name__ == "__main__":
    main()
