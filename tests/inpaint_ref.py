"""CPU restatement of the inpainting generation program (tests/test_sdxl_zh_inpaint.py `StableDiffusionTest.__call__`,
:481-762, 9-channel UNet, no denoising_start) on the fp32 oracles: oracle.unet_ref, oracle.vae_ref, oracle.sampler_ref.
Test infrastructure only (tests/test_inpaint_*.py)."""
import torch
import torch.nn.functional as F

from oracle.sampler_ref import cfg_combine_ref, rescale_noise_cfg_ref


def prepare_ref(image, mask):
    """VaeImageProcessor.preprocess (normalise, binarise), the masking of :590, prepare_mask_latents' nearest resize"""
    init = 2.0 * image - 1.0
    m = mask.clone()
    m[m < 0.5] = 0
    m[m >= 0.5] = 1
    masked = init * (m < 0.5)
    lmask = F.interpolate(m, size=(image.shape[2] // 8, image.shape[3] // 8))
    return init, masked, lmask


def get_timesteps_ref(timesteps, n, strength):
    init_timestep = min(int(n * strength), n)
    t_start = max(n - init_timestep, 0)
    return timesteps[t_start:], n - t_start, t_start


def inpaint_denoise_ref(unet, scheduler, vae, image, mask, prompt_embeds, added_cond_kwargs, num_inference_steps,
                        strength, guidance_scale, guidance_rescale, noise, vae_noise):
    """-> final latents.  vae_noise = (init image, masked image) posterior noise; `unet` takes the 9-channel input."""
    do_cfg = guidance_scale > 1.0
    scheduler.set_timesteps(num_inference_steps)
    timesteps, left, t_start = get_timesteps_ref(scheduler.timesteps, num_inference_steps, strength)
    assert left >= 1
    scheduler.step_index = t_start               # diffusers 0.23: the index of timesteps[t_start] in the full schedule
    init, masked, lmask = prepare_ref(image, mask)
    sf = vae.config.scaling_factor
    if strength == 1.0:
        latents = noise * scheduler.init_noise_sigma
    else:
        image_latents = vae.encode(init).latent_dist.sample(noise=vae_noise[0]) * sf
        ac = torch.tensor(scheduler.alphas_cumprod, dtype=torch.float32)[int(timesteps[0])]
        latents = ac.sqrt() * image_latents + (1 - ac).sqrt() * noise
    masked_latents = vae.encode(masked).latent_dist.sample(noise=vae_noise[1]) * sf
    m2 = torch.cat([lmask] * 2) if do_cfg else lmask
    ml2 = torch.cat([masked_latents] * 2) if do_cfg else masked_latents
    for t in timesteps:
        x = torch.cat([latents] * 2) if do_cfg else latents
        x = torch.cat([x, m2, ml2], dim=1)
        eps = unet(x, int(t), encoder_hidden_states=prompt_embeds, added_cond_kwargs=added_cond_kwargs,
                   return_dict=False)[0]
        if do_cfg:
            eps, eps_text = cfg_combine_ref(eps, guidance_scale)
            if guidance_rescale > 0.0:
                eps = rescale_noise_cfg_ref(eps, eps_text, guidance_rescale)
        latents = scheduler.step(eps, t, latents)[0]
    return latents
