"""SDXL inpainting on the HIP path: the generation program of tests/test_sdxl_zh_inpaint.py
(`StableDiffusionTest.__call__`, :481-762) after the prompt encoding.  Input preparation (`VaeImageProcessor.preprocess`,
the masking of :590 and `prepare_mask_latents` :307-358) is one HIP kernel (`ops.inpaint_prepare`); the VAE encodes are
`HipVAEEncoder.encode_latents`; the UNet is a 9-channel `HipUNet(..., inpaint_inputs=True)` whose conv_in gathers the
latents, the mask and the masked-image latents itself, so the loop body hands it the latents alone instead of the
reference's two per-step concatenations.  Host-side image decoding and resizing (PIL) stay outside: image and mask arrive
as tensors of the output size, a multiple of 8 on each side."""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import torch

from . import ops


def prepare_mask_and_masked_image(image: torch.Tensor, mask: torch.Tensor):
    """image fp32 [N,3,8h,8w], mask fp32 [N,1,8h,8w], both in [0, 1] ->
    (init_image = 2 image - 1, masked_image = init_image * (mask < 0.5), latent_mask = binarised mask at [N,1,h,w])"""
    if image.dim() != 4 or image.shape[1] != 3 or mask.dim() != 4 or mask.shape[1] != 1 or \
            image.shape[0] != mask.shape[0] or image.shape[2:] != mask.shape[2:]:
        raise ValueError(f"image {tuple(image.shape)} / mask {tuple(mask.shape)}: expected [N,3,H,W] / [N,1,H,W]")
    if image.shape[2] % 8 or image.shape[3] % 8:
        raise ValueError(f"image size {tuple(image.shape[2:])} must be a multiple of 8 (resize on the host first)")
    dev = torch.device("cuda", torch.cuda.current_device())
    image = image.detach().to(dev, torch.float32).contiguous()
    mask = mask.detach().to(dev, torch.float32).contiguous()
    return ops.inpaint_prepare(image, mask)


def get_timesteps(scheduler, num_inference_steps: int, strength: float):
    """:383-417 without `denoising_start`: -> (timesteps[t_start:], steps left, t_start).  `set_timesteps` must have run."""
    n = num_inference_steps
    init_timestep = min(int(n * strength), n)
    t_start = max(n - init_timestep, 0)
    timesteps = scheduler.timesteps[t_start * scheduler.order:]
    left = n - t_start
    if left < 1:
        raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline "
                         f"steps is {left} which is < 1 and not appropriate for this pipeline.")
    return timesteps, left, t_start


def _noise(shape, noise, generator, device):
    if noise is not None:
        if tuple(noise.shape) != tuple(shape):
            raise ValueError(f"noise {tuple(noise.shape)} != {tuple(shape)}")
        return noise.to(device, torch.float32).contiguous()
    return torch.randn(shape, generator=generator, device=device, dtype=torch.float32)


def inpaint_denoise(unet, scheduler, vae_encoder, image, mask, prompt_embeds, added_cond_kwargs,
                    num_inference_steps: int = 50, strength: float = 0.9999, guidance_scale: float = 7.5,
                    guidance_rescale: float = 0.0, noise: Optional[torch.Tensor] = None,
                    vae_noise: Optional[Sequence[Optional[torch.Tensor]]] = None, generator: Optional[torch.Generator] = None,
                    callback: Optional[Callable] = None, timestep_cond=None) -> torch.Tensor:
    """Inpainting denoise loop (:481-762) -> final latents fp32 [N,4,h,w] (the VAE decode stays outside, as in
    `sampler.denoise`).  image / mask: [N,3,8h,8w] / [N,1,8h,8w] in [0, 1]; `unet` a 9-channel HipUNet built with
    inpaint_inputs=True for batch 2N under CFG (guidance_scale > 1), N otherwise; `vae_encoder` a HipVAEEncoder for [N,3,8h,8w].
    noise: the start noise [N,4,h,w]; vae_noise: (init image, masked image) posterior-sampling noise of the two VAE encodes
    (the first is only used when strength < 1).  Anything not given is drawn from `generator` in the reference's order:
    init-image encode, start noise, masked-image encode.  The sigma-space schedulers (`sampler.EulerDiscrete`, ...) start a
    strength < 1 run from `image_latents + sigma * noise` and get `generator` for their steps; `timestep_cond` as in
    `sampler.denoise`."""
    from .sampler import check_timestep_cond
    if unet.in_channels == unet.cfg.out_channels:
        raise ValueError(f"inpaint_denoise needs a {2 * unet.cfg.out_channels + 1}-channel inpainting UNet; a "
                         f"{unet.in_channels}-channel UNet never sees the mask (that is img2img)")
    if unet.in_channels != 2 * unet.cfg.out_channels + 1:
        raise ValueError(f"The unet should have either 4 or 9 input channels, not {unet.in_channels}.")
    if not getattr(unet, "inpaint_inputs", False):
        raise ValueError("inpaint_denoise: build the UNet with HipUNet(..., inpaint_inputs=True)")
    do_cfg = guidance_scale > 1.0
    timestep_cond = check_timestep_cond(unet, timestep_cond, do_cfg)
    ukw = {} if timestep_cond is None else dict(timestep_cond=timestep_cond)
    skw = dict(generator=generator) if getattr(scheduler, "fused_model_input", False) else {}
    N = image.shape[0]
    if unet.B != (2 * N if do_cfg else N):
        raise ValueError(f"The UNet is built for batch {unet.B}; {N} images {'with' if do_cfg else 'without'} CFG need "
                         f"{2 * N if do_cfg else N}")
    vn = list(vae_noise) if vae_noise is not None else [None, None]
    scheduler.set_timesteps(num_inference_steps)
    timesteps, _, t_start = get_timesteps(scheduler, num_inference_steps, strength)
    scheduler.set_begin_index(t_start)
    is_strength_max = strength == 1.0
    init_image, masked_image, latent_mask = prepare_mask_and_masked_image(image, mask)
    dev = init_image.device
    shape = (N, unet.cfg.out_channels, unet.H, unet.W)
    if tuple(latent_mask.shape[2:]) != shape[2:]:
        raise ValueError(f"image {tuple(image.shape[2:])} does not match the UNet's latent size {shape[2:]} x 8")
    image_latents = None
    if not is_strength_max:
        image_latents = vae_encoder.encode_latents(init_image, noise=_noise(shape, vn[0], generator, dev))
    noise = _noise(shape, noise, generator, dev)
    if is_strength_max:
        latents = (noise * scheduler.init_noise_sigma).contiguous()
    else:
        t0 = timesteps[:1].to(dev, torch.int64).repeat(N).contiguous()
        ac = torch.from_numpy(scheduler.alphas_cumprod).to(dev, torch.float32)
        if getattr(scheduler, "fused_model_input", False):
            latents = scheduler.add_noise(image_latents, noise, t_start)
        else:
            latents = ops.add_noise(image_latents.contiguous(), noise, t0, ac)
    masked_latents = vae_encoder.encode_latents(masked_image, noise=_noise(shape, vn[1], generator, dev))
    unet.set_inpaint_cond(latent_mask, masked_latents, latent_batch=N)
    try:
        for i, t in enumerate(timesteps):
            x = scheduler.scale_model_input(latents, t)
            noise_pred = unet(x, t, encoder_hidden_states=prompt_embeds, added_cond_kwargs=added_cond_kwargs,
                              return_dict=False, **ukw)[0]
            if do_cfg:
                noise_pred = ops.cfg_combine(noise_pred.float(), guidance_scale, guidance_rescale)
            latents = scheduler.step(noise_pred, t, latents, return_dict=False, **skw)[0]
            if callback is not None:
                callback(i, t, latents)
    finally:
        unet.clear_inpaint_cond()
    return latents
