"""CPU restatement of the LCM few-step sampler (tests/test_sdxl_zh_lcm.py:178 `LCMScheduler.from_config(...)`, the loop of
:407-430 at guidance_scale 0) in float64, written from the scheduler's formulas: scaled-linear betas 0.00085-0.012 over 1000
training steps, epsilon prediction, original_inference_steps 50, boundary scalings with sigma_data 0.5 and timestep scaling
10.  Test infrastructure only (tests/test_lcm_*.py, tests/test_lora_gpu.py)."""
import math

import torch


class LCMSchedulerRef:
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, original_inference_steps=50):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float64) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.T, self.orig = num_train_timesteps, original_inference_steps
        self.timesteps = None

    def set_timesteps(self, n):
        c = self.T // self.orig
        origin = [(j + 1) * c - 1 for j in range(self.orig)]
        skip = self.orig // n
        self.timesteps = torch.tensor(origin[::-skip][:n], dtype=torch.int64)
        self.step_index = 0
        return self.timesteps

    def scale_model_input(self, sample, timestep=None):
        return sample

    @staticmethod
    def scalings(t):
        s = 10.0 * float(t)
        return 0.25 / (s * s + 0.25), s / math.sqrt(s * s + 0.25)

    def scalars(self, i):
        """(a_t, a_prev, c_skip, c_out) of step i; a_prev behind the last timestep is alphas_cumprod[0]"""
        t = int(self.timesteps[i])
        nxt = int(self.timesteps[i + 1]) if i + 1 < len(self.timesteps) else 0
        c_skip, c_out = self.scalings(t)
        return float(self.alphas_cumprod[t]), float(self.alphas_cumprod[nxt]), c_skip, c_out

    def step(self, eps, timestep, sample, generator=None, noise=None):
        """-> (prev_sample, denoised) in float64"""
        i = self.step_index
        assert int(timestep) == int(self.timesteps[i])
        a_t, a_prev, c_skip, c_out = self.scalars(i)
        x, eps = sample.double(), eps.double()
        x0 = (x - math.sqrt(1.0 - a_t) * eps) / math.sqrt(a_t)
        denoised = c_out * x0 + c_skip * x
        if i == len(self.timesteps) - 1:
            out = denoised
        else:
            if noise is None:
                noise = torch.randn(sample.shape, generator=generator, dtype=torch.float32)
            out = math.sqrt(a_prev) * denoised + math.sqrt(1.0 - a_prev) * noise.double()
        self.step_index += 1
        return out, denoised


def lcm_denoise_ref(unet, scheduler, latents, prompt_embeds, added_cond_kwargs, num_inference_steps, generator=None,
                    calls=None):
    """the generation loop at guidance_scale 0: one UNet evaluation at batch B per step, noise from `generator` between
    steps; `unet` works in fp32 (the oracle UNet), the scheduler in float64.  `calls` collects the batch of every call."""
    scheduler.set_timesteps(num_inference_steps)
    latents = latents.double() * scheduler.init_noise_sigma
    for t in scheduler.timesteps:
        x = scheduler.scale_model_input(latents, t)
        if calls is not None:
            calls.append(x.shape[0])
        eps = unet(x.float(), int(t), encoder_hidden_states=prompt_embeds, added_cond_kwargs=added_cond_kwargs,
                   return_dict=False)[0]
        latents = scheduler.step(eps, t, latents, generator=generator)[0]
    return latents
