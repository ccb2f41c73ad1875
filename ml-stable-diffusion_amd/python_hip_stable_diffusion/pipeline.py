"""``HipStableDiffusionPipeline`` - the reference's generation loop over MI355X model runners.

Mirrors ``CoreMLStableDiffusionPipeline`` (python_coreml_stable_diffusion/pipeline.py:47-589):
same constructor arguments, same ``__call__`` arguments and semantics (prompt, height/width
taken from the model, num_inference_steps, guidance_scale, negative_prompt, latents,
callback/callback_steps, controlnet_cond, SDXL size conditioning, unet_batch_one), same
tensor hand-offs to the model runners; ``get_hip_pipe`` / ``main`` mirror ``get_coreml_pipe`` /
``main`` (pipeline.py:607-697, :724-858) over a diffusers checkpoint directory instead of converted
``.mlpackage`` files.  Differences, all additive:
  * model runners are ``HipModel`` objects (``libsdmi355.so``) instead of ``CoreMLModel``;
  * when no per-step callback is requested and the scheduler exports linear tables, the whole loop
    (pipeline.py:500-573) - ControlNets included - runs device-resident in one call
    (``sd_unet_denoise_loop``); otherwise it steps through the boundary exactly like the reference
    and says so in one log line;
  * several prompts / several images per prompt are generated in one batched loop like the Swift
    pipeline's ``imageCount`` (StableDiffusionPipeline.swift:233-333) - the Python reference refuses
    them (pipeline.py:434-438); the UNet handle must have been built for that batch;
  * an SDXL refiner UNet takes over at step ``int(N * refiner_start)`` with its own conditioning
    (StableDiffusionXLPipeline.swift:205-225, :326-358);
  * ``seed`` is an argument (the reference seeds numpy globally in ``main``, pipeline.py:726) and
    the initial latents come from the bit-exact numpy legacy stream implemented in the library
    (``sd_numpy_randn``), so results do not depend on global RNG state;
  * image-to-image, the Swift pipeline's ``startingImage`` / ``strength`` (StableDiffusionPipeline.Configuration.swift:22-26,
    :74-80; StableDiffusionPipeline.swift:242-262, :361-379; CLI ``--image`` / ``--strength``): the starting image goes through a
    VAE encoder handle, its posterior sample is noised to the first timestep of the truncated schedule on the device
    (``HipVaeEncoder.encode_latents``) and the loop runs over the schedule's tail;
  * a progress handler, the Swift pipeline's ``sample(configuration:progressHandler:)`` (StableDiffusionPipeline.swift:205-210,
    :332-349, :411-426; ``useDenoisedIntermediates`` Configuration.swift:43-44; CLI ``--save-every``, StableDiffusionCLI/main.swift:57-63,
    :260-263): ``progress_handler(PipelineProgress)`` runs after every ``progress_steps``-th step, gets the latents or the scheduler's
    de-noised estimate with lazily decoded preview images, and stops the generation by returning False.  Unlike ``callback`` it
    keeps the loop device-resident: the handler runs between two graph replays of ``sd_unet_denoise_loop_progress``;
  * ``device_postprocess`` (CLI ``--device-postprocess``; off by default): the final decode and every preview go from the
    decoder's last conv to the 8-bit image and the safety verdict on the device (``sd_vae_decode_images``, csrc/imgpost.hip) instead of
    through numpy, PIL and CLIPImageProcessor on the host (pipeline.py:286-320); the results are bit for bit the host route's;
  * ``--attention-implementation`` is a run-time flag of ``main`` (a conversion-time flag in the
    reference, torch2coreml.py:1678-1685).
"""
import argparse
import inspect
import json
import logging
import os
from types import SimpleNamespace

import numpy as np

from . import _lib
from .schedulers import SCHEDULER_MAP, get_available_schedulers  # noqa: F401  (pipeline.py:592-604)

logger = logging.getLogger(__name__)
VAE_DECODER_UPSAMPLE_FACTOR = 8          # pipeline.py:108
VAE_SCALING_FACTOR = 0.18215             # pipeline.py:314 (SD 1.x / 2.x); SDXL 0.13025 (main.swift:124)


class PipelineProgress:
    """What the progress handler receives after a step (``PipelineProgress``, StableDiffusionPipeline.swift:411-426): ``pipeline``,
    ``prompt``, ``step`` (index into the timestep list, over both stages with a refiner), ``step_count`` (the list's length: PNDM's
    doubled entry counts, like Swift's ``timeSteps.count``), ``current_latent_samples`` (n_images, C, H, W) float32 - the de-noised
    estimate with ``use_denoised_intermediates``, else the latents - and ``current_images``, decoded from them on first access
    (``decodeToImages``: the VAE decoder, then the safety checker) in the call's ``output_type``."""

    def __init__(self, pipeline, prompt, step, step_count, current_latent_samples, output_type="np"):
        self.pipeline, self.prompt, self.step, self.step_count = pipeline, prompt, step, step_count
        self.current_latent_samples = current_latent_samples
        self._output_type, self._images = output_type, None

    @property
    def current_images(self):
        if self._images is None:
            if self.pipeline.vae_decoder is None:
                raise ValueError("current_images needs a pipeline with a VAE decoder")
            if self.pipeline.device_postprocess:
                self._images, _ = self.pipeline.decode_images_on_device(self.current_latent_samples, self._output_type)
            else:
                image, _ = self.pipeline.run_safety_checker(self.pipeline.decode_latents(self.current_latent_samples))
                self._images = self.pipeline.numpy_to_pil(image) if self._output_type == "pil" else image
        return self._images


class HipStableDiffusionPipeline:
    def __init__(self, text_encoder, unet, vae_decoder, scheduler, tokenizer, controlnet=None, xl=False,
                 force_zeros_for_empty_prompt=True, feature_extractor=None, safety_checker=None,
                 text_encoder_2=None, tokenizer_2=None, vae_scaling_factor=None, unet_refiner=None,
                 refiner_start=0.8, aesthetic_score=6.0, negative_aesthetic_score=2.5, vae_encoder=None, device_postprocess=False):
        self.text_encoder, self.text_encoder_2 = text_encoder, text_encoder_2
        self.tokenizer, self.tokenizer_2 = tokenizer, tokenizer_2
        self.unet, self.vae_decoder, self.scheduler = unet, vae_decoder, scheduler
        self.vae_encoder = vae_encoder                       # image-to-image only (Encoder.swift); None: text-to-image only
        self.controlnet = controlnet
        self.xl = xl
        self.force_zeros_for_empty_prompt = force_zeros_for_empty_prompt
        self.feature_extractor, self.safety_checker = feature_extractor, safety_checker
        self.vae_scaling_factor = vae_scaling_factor or (0.13025 if xl else VAE_SCALING_FACTOR)
        # SDXL base -> refiner hand-off (StableDiffusionXLPipeline.swift:37-41, Configuration defaults)
        self.unet_refiner, self.refiner_start = unet_refiner, refiner_start
        self.aesthetic_score, self.negative_aesthetic_score = aesthetic_score, negative_aesthetic_score
        if safety_checker is None:
            logger.warning("safety checker disabled for %s", type(self).__name__)
        elif feature_extractor is None:                                              # pipeline.py:288 needs it
            raise ValueError("a safety checker needs the checkpoint's feature extractor (CLIPImageProcessor) for its input")
        # static shapes come from the model, like the reference (pipeline.py:104-117)
        self.unet.in_channels = self.unet.expected_inputs["sample"]["shape"][1]
        latent_h, latent_w = self.unet.expected_inputs["sample"]["shape"][2:]
        self.height = latent_h * VAE_DECODER_UPSAMPLE_FACTOR
        self.width = latent_w * VAE_DECODER_UPSAMPLE_FACTOR
        logger.info("Stable Diffusion configured to generate %dx%d images", self.height, self.width)
        self.device_postprocess, self._image_post = bool(device_postprocess), None
        if self.device_postprocess:
            self._image_post = self._check_device_postprocess()

    def _check_device_postprocess(self):
        """``device_postprocess`` drives library handles: anything else is refused here, not worked around later."""
        from .hip_model import HipVaeDecoder
        from .safety_checker import HipSafetyChecker, image_post
        if not isinstance(self.vae_decoder, HipVaeDecoder):
            raise ValueError(f"device_postprocess needs a HipVaeDecoder handle, got {type(self.vae_decoder).__name__}")
        if self.safety_checker is None:
            return None
        if not isinstance(self.safety_checker, HipSafetyChecker):
            raise ValueError(f"device_postprocess needs a HipSafetyChecker handle (or no checker), got {type(self.safety_checker).__name__}")
        if self.vae_decoder.batch % self.safety_checker.batch:
            raise ValueError(f"device_postprocess: the VAE decoder's static batch of {self.vae_decoder.batch} is no multiple of the "
                             f"safety checker's {self.safety_checker.batch}")
        _, _, h, w = self.vae_decoder.image_shape
        return image_post(self.feature_extractor, h, w, self.safety_checker.image_size)

    # ---- pipeline.py:123-257 ---------------------------------------------------------------
    def _encode_prompt(self, prompt, prompt_2=None, do_classifier_free_guidance=True, negative_prompt=None,
                       negative_prompt_2=None, for_refiner=False):
        batch_size = len(prompt) if isinstance(prompt, list) else 1
        if self.xl:
            prompts = [prompt, prompt_2 if prompt_2 is not None else prompt]
            if self.tokenizer is not None and not for_refiner:
                tokenizers, encoders = [self.tokenizer, self.tokenizer_2], [self.text_encoder, self.text_encoder_2]
            else:   # refiner: only tokenizer_2 / text_encoder_2 (pipeline.py:134-141; ...XLPipeline.swift:262-270)
                prompts, tokenizers, encoders = prompts[1:], [self.tokenizer_2], [self.text_encoder_2]
            key = "hidden_embeds"
        else:
            prompts, tokenizers, encoders, key = [prompt], [self.tokenizer], [self.text_encoder], "last_hidden_state"

        def encode(texts):
            embeds, pooled = [], None
            for text, tok, enc in zip(texts, tokenizers, encoders):
                ids = tok(text, padding="max_length", max_length=tok.model_max_length, truncation=True,
                          return_tensors="np").input_ids
                ids = np.asarray(ids).reshape(-1, ids.shape[-1])
                rows = [enc(input_ids=ids[i:i + 1].astype(np.float32)) for i in range(ids.shape[0])]   # ids as float32 (:173)
                embeds.append(np.concatenate([r[key] for r in rows]))
                if self.xl:
                    pooled = np.concatenate([r["pooled_outputs"] for r in rows])
            return np.concatenate(embeds, axis=-1), pooled

        prompt_embeds, pooled = encode(prompts)
        if do_classifier_free_guidance:
            if negative_prompt is None and self.force_zeros_for_empty_prompt:        # pipeline.py:183-187
                neg, neg_pooled = np.zeros_like(prompt_embeds), (np.zeros_like(pooled) if self.xl else None)
            else:
                negative_prompt = negative_prompt or ""
                negative_prompt_2 = negative_prompt_2 or negative_prompt
                if isinstance(prompt, list) and not isinstance(negative_prompt, list):
                    negative_prompt = batch_size * [negative_prompt]
                    negative_prompt_2 = batch_size * [negative_prompt_2]
                if type(prompt) is not type(negative_prompt):
                    raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got "
                                    f"{type(negative_prompt)} != {type(prompt)}.")
                if isinstance(negative_prompt, list) and len(negative_prompt) != batch_size:
                    raise ValueError("`negative_prompt` batch size does not match `prompt`")
                negs = [negative_prompt, negative_prompt_2]
                neg, neg_pooled = encode(negs[1:] if (self.xl and len(tokenizers) == 1) else negs[:len(tokenizers)])
            prompt_embeds = np.concatenate([neg, prompt_embeds])                     # [uncond, cond] (:245)
            if self.xl:
                pooled = np.concatenate([neg_pooled, pooled])
        return prompt_embeds.transpose(0, 2, 1)[:, :, None, :], pooled             # (B, C, 1, 77) (:252)

    # ---- pipeline.py:259-284 ---------------------------------------------------------------
    def run_controlnet(self, sample, timestep, encoder_hidden_states, controlnet_cond):
        if not self.controlnet:
            raise ValueError("Conditions for controlnet are given but the pipeline has no controlnet modules")
        if len(controlnet_cond) != len(self.controlnet):
            raise ValueError(f"need {len(self.controlnet)} controlnet conditions, got {len(controlnet_cond)}")
        total = None
        for cn, cond in zip(self.controlnet, controlnet_cond):
            out = cn(sample=sample.astype(np.float16), timestep=timestep.astype(np.float16),
                     encoder_hidden_states=encoder_hidden_states.astype(np.float16), controlnet_cond=cond)
            total = out if total is None else {k: total[k] + v for k, v in out.items()}
        return {k: v.astype(np.float16) for k, v in total.items()}

    # ---- pipeline.py:286-311 ---------------------------------------------------------------
    def run_safety_checker(self, image):
        if self.safety_checker is None:
            return image, None
        clip_input = self.feature_extractor(self.numpy_to_pil(image), return_tensors="np").pixel_values.astype(np.float16)
        sb = self.safety_checker.expected_inputs["clip_input"]["shape"][0]
        # the checker handle has a static batch like every model (pipeline.py:112-114): feed it in slices
        if image.shape[0] % sb:
            raise ValueError(f"{image.shape[0]} images do not fill the safety checker's static batch of {sb}")
        outs = [self.safety_checker(clip_input=np.ascontiguousarray(clip_input[i:i + sb]),
                                    images=np.ascontiguousarray(image[i:i + sb]).astype(np.float16),
                                    adjustment=np.array([0.]).astype(np.float16))    # defaults to 0 in the original pipeline
                for i in range(0, image.shape[0], sb)]
        has_nsfw = np.concatenate([np.asarray(o["has_nsfw_concepts"]).reshape(-1) for o in outs])
        # filtered_images without the detour through the checker's float16 input: unflagged images stay bit for bit what the
        # VAE produced, flagged ones are zeroed like the model's output
        filtered = image.copy()
        filtered[has_nsfw.astype(bool)] = 0
        logger.info("Generated image has nsfw concept=%s", bool(has_nsfw.any()))
        return filtered, has_nsfw

    # ---- pipeline.py:313-320 ---------------------------------------------------------------
    def decode_latents(self, latents):
        latents = 1 / self.vae_scaling_factor * latents
        dtype = self.vae_decoder.expected_inputs["z"]["dtype"]
        vb = self.vae_decoder.expected_inputs["z"]["shape"][0]
        # the decoder handle has a static batch like every model (pipeline.py:112-114): feed it in slices
        if latents.shape[0] % vb:
            raise ValueError(f"{latents.shape[0]} latents do not fill the VAE decoder's static batch of {vb}")
        image = np.concatenate([self.vae_decoder(z=np.ascontiguousarray(latents[i:i + vb]).astype(dtype))["image"]
                                for i in range(0, latents.shape[0], vb)])
        image = np.clip(image / 2 + 0.5, 0, 1)
        return image.transpose((0, 2, 3, 1))

    def decode_images_on_device(self, latents, output_type):
        """decode_latents + run_safety_checker (+ numpy_to_pil) through ``HipVaeDecoder.decode_images``: (images, has_nsfw).
        ``output_type="pil"``: PIL images straight from the device's 8-bit image, no fp32 read-back; else the float images (n, H, W, 3)
        in [0, 1], computed from the decoder's output as decode_latents does.  Flagged images are black either way."""
        latents = 1 / self.vae_scaling_factor * latents
        dtype = self.vae_decoder.expected_inputs["z"]["dtype"]
        vb = self.vae_decoder.expected_inputs["z"]["shape"][0]
        if latents.shape[0] % vb:
            raise ValueError(f"{latents.shape[0]} latents do not fill the VAE decoder's static batch of {vb}")
        pil = output_type == "pil"
        outs = [self.vae_decoder.decode_images(np.ascontiguousarray(latents[i:i + vb]).astype(dtype), self.safety_checker,
                                               self._image_post, want_image=not pil, want_rgb8=pil)
                for i in range(0, latents.shape[0], vb)]
        has_nsfw = None
        if self.safety_checker is not None:
            has_nsfw = np.concatenate([o["has_nsfw_concepts"] for o in outs])
            logger.info("Generated image has nsfw concept=%s", bool(has_nsfw.any()))
        if pil:
            from PIL import Image
            return [Image.fromarray(im) for o in outs for im in o["rgb8"]], has_nsfw
        image = np.clip(np.concatenate([o["image"] for o in outs]) / 2 + 0.5, 0, 1).transpose((0, 2, 3, 1))
        if has_nsfw is not None:
            image[has_nsfw] = 0                              # the library zeroed them in [-1, 1], which is mid-grey here
        return image, has_nsfw

    # ---- pipeline.py:322-344 ---------------------------------------------------------------
    def prepare_latents(self, batch_size, num_channels_latents, height, width, latents=None, seed=None, rng="numpy"):
        """``rng``: which of the reference's seed-exact sources draws the latents (RandomSource.swift, CLI --rng):
        "numpy" (np.random.seed + randn, the Python pipeline's), "torch" (torch CPU generator), "nvidia" (torch CUDA
        generator, Philox)."""
        shape = (batch_size, num_channels_latents, self.height // 8, self.width // 8)
        if latents is None:
            n = int(np.prod(shape))
            if seed is None:
                latents = np.random.randn(*shape).astype(np.float16)           # reference behaviour (:331)
            elif rng == "numpy":
                latents = _lib.numpy_randn(int(seed), n).reshape(shape).astype(np.float16)
            elif rng == "torch":
                latents = _lib.torch_randn(int(seed), n).reshape(shape).astype(np.float16)
            elif rng == "nvidia":
                latents = _lib.philox_randn(int(seed), n).reshape(shape).astype(np.float16)
            else:
                raise ValueError(f"rng must be 'numpy', 'torch' or 'nvidia', got {rng!r}")
        elif latents.shape != shape:
            raise ValueError(f"Unexpected latents shape, got {latents.shape}, expected {shape}")
        return latents * np.float32(self.scheduler.init_noise_sigma)

    def prepare_image_latents(self, starting_image, strength, num_inference_steps, batch_size, num_channels_latents,
                              latents=None, seed=None, rng="numpy"):
        """Image-to-image start (generateLatentSamples, StableDiffusionPipeline.swift:361-379): truncates the schedule
        (``scheduler.set_timesteps(n, strength)``) and returns the ``batch_size`` starting latents, float32 - the posterior sample
        of the encoded image times the scale factor (Encoder.swift:48-92), noised to the first timestep of the tail
        (Scheduler.swift:83-102).  Draw order of the reference: unit-variance noise for every latent first (user ``latents`` take
        their place), then the posterior normals from the same source.  ``rng="numpy"``: one continued stream
        (NumPyRandomSource.swift:86-117: normalShapedArray is consecutive nextNormal draws).  ``rng="nvidia"``: every array and
        every single nextNormal is one Philox launch with its own offset (NvRandomSource.swift:65-90): image i is offset i, the
        j-th posterior normal offset batch_size + j.  ``rng="torch"``: the posterior draws continue the generator behind the
        vectorised array draw (TorchRandomSource.swift:94-150), which ``sd_torch_randn`` does not export - NotImplementedError.
        The noise is NOT scaled by ``init_noise_sigma``: the add-noise coefficients carry the level."""
        if self.vae_encoder is None:                                               # startingImageProvidedWithoutEncoder
            raise ValueError("a starting image needs a VAE encoder: build the pipeline with vae_encoder=...")
        if rng not in ("numpy", "torch", "nvidia"):
            raise ValueError(f"rng must be 'numpy', 'torch' or 'nvidia', got {rng!r}")
        if rng == "torch" and seed is not None:
            raise NotImplementedError("image-to-image with rng='torch': the posterior normals continue torch's CPU generator behind "
                                      "the latents' array draw, and sd_torch_randn exports whole arrays from a fresh seed only")
        enc = self.vae_encoder.expected_inputs["x"]
        x = np.asarray(starting_image)
        if x.ndim == 3:
            x = x[None]
        if x.shape != tuple(enc["shape"]) or enc["shape"][0] != 1:                 # Encoder.swift:57-60 sampleInputShapeNotCorrect
            raise ValueError(f"Unexpected starting image shape, got {np.asarray(starting_image).shape}, expected "
                             f"{tuple(enc['shape'][1:])} (the encoder handle has batch {enc['shape'][0]}, must be 1)")
        shape = (batch_size, num_channels_latents, self.height // 8, self.width // 8)
        n_noise, n_post = int(np.prod(shape)), int(np.prod(shape[1:]))
        if latents is not None and latents.shape != shape:
            raise ValueError(f"Unexpected latents shape, got {latents.shape}, expected {shape}")
        if rng == "nvidia" and seed is not None:
            noise = latents if latents is not None else np.stack(
                [_lib.philox_randn(int(seed), n_post, offset=i).reshape(shape[1:]) for i in range(batch_size)])
            eps = np.array([_lib.philox_randn(int(seed), 1, offset=batch_size + j)[0] for j in range(n_post)]).reshape(shape[1:])
        else:
            stream = (np.random.randn(n_noise + n_post) if seed is None            # reference behaviour: numpy's global stream
                      else _lib.numpy_randn(int(seed), n_noise + n_post))
            noise = stream[:n_noise].reshape(shape) if latents is None else latents
            eps = stream[n_noise:].reshape(shape[1:])
        self.scheduler.set_timesteps(num_inference_steps, strength)
        sa, sb = self.scheduler.add_noise_coefficients()
        return self.vae_encoder.encode_latents(np.ascontiguousarray(x.astype(enc["dtype"])), eps.astype(np.float32),
                                               np.ascontiguousarray(noise, dtype=np.float32), self.vae_scaling_factor, sa, sb)

    def prepare_control_cond(self, controlnet_cond, do_classifier_free_guidance, batch_size, num_images_per_prompt):
        out = []
        for cond in controlnet_cond:                                              # pipeline.py:346-357
            cond = np.stack([cond] * batch_size * num_images_per_prompt)
            if do_classifier_free_guidance:
                cond = np.concatenate([cond] * 2)
            out.append(cond.astype(np.float16))
        return out

    def check_inputs(self, prompt, height, width, callback_steps):
        if height != self.height or width != self.width:                          # pipeline.py:359-365
            logger.warning("image %dx%d is fixed by the model; requested %sx%s ignored", self.height, self.width,
                           height, width)
        if not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if self.height % 8 != 0 or self.width % 8 != 0:
            raise ValueError("`height` and `width` have to be divisible by 8")
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps}")

    def prepare_extra_step_kwargs(self, eta):
        """pipeline.py:384-396: eta is forwarded only to schedulers whose ``step`` accepts it (DDIM)."""
        accepts_eta = "eta" in set(inspect.signature(self.scheduler.step).parameters.keys())
        return {"eta": eta} if accepts_eta else {}

    @staticmethod
    def _get_add_time_ids(original_size, crops_coords_top_left, target_size, dtype):
        return np.array(list(original_size + crops_coords_top_left + target_size)).astype(dtype)   # :398-401

    def _xl_kwargs(self, model, pooled, original_size, crops_coords_top_left, target_size, do_cfg, n_img, refiner):
        """SDXL micro-conditioning (pipeline.py:458-472); refiner geometry + aesthetic scores for the
        [uncond, cond] halves (StableDiffusionXLPipeline.swift:326-358)."""
        if refiner:
            neg = np.array(list(original_size + crops_coords_top_left) + [self.negative_aesthetic_score], np.float32)
            pos = np.array(list(original_size + crops_coords_top_left) + [self.aesthetic_score], np.float32)
            ids = np.concatenate([np.tile(neg, (n_img, 1)), np.tile(pos, (n_img, 1))]) if do_cfg else np.tile(pos, (n_img, 1))
        else:
            ids = self._get_add_time_ids(tuple(original_size), tuple(crops_coords_top_left), tuple(target_size), np.float32)
            if len(model.expected_inputs["time_ids"]["shape"]) > 1:
                ids = np.tile(ids[None], ((2 if do_cfg else 1) * n_img, 1))
            else:                                              # legacy flat (12,) layout (:466)
                ids = np.concatenate([ids] * ((2 if do_cfg else 1) * n_img))
        return {"text_embeds": pooled.astype(np.float16), "time_ids": ids.astype(np.float16)}

    @staticmethod
    def _per_image(emb, n_prompts, num_images_per_prompt, cfg_mul):
        """(cfg*P, ...) [uncond P | cond P] -> (cfg*P*n, ...) with every prompt's rows repeated n times."""
        if emb is None or num_images_per_prompt == 1:
            return emb
        halves = np.split(emb, cfg_mul)
        return np.concatenate([np.repeat(h, num_images_per_prompt, axis=0) for h in halves])

    # ---- pipeline.py:403-589 ---------------------------------------------------------------
    def __call__(self, prompt, height=512, width=512, num_inference_steps=50, guidance_scale=7.5, negative_prompt=None,
                 num_images_per_prompt=1, eta=0.0, latents=None, output_type="np", return_dict=True, callback=None,
                 callback_steps=1, controlnet_cond=None, original_size=None, crops_coords_top_left=(0, 0),
                 target_size=None, unet_batch_one=False, seed=None, device_loop=True, rng="numpy", starting_image=None,
                 strength=1.0, progress_handler=None, progress_steps=1, use_denoised_intermediates=False, **kwargs):
        """``progress_handler(PipelineProgress)``: called after every step i with ``i % progress_steps == 0``; a falsy return other
        than None stops the generation (``images == []``, ``cancelled=True``, ``latents`` at the stop); it does not move the loop off
        the device.  ``use_denoised_intermediates``: its ``current_latent_samples`` are the scheduler's de-noised estimate.
        ``starting_image`` (3, H, W) or (1, 3, H, W) in [-1, 1] with ``strength`` < 1.0: image-to-image - the fraction
        ``strength`` of the schedule runs, from the encoded image noised to its first timestep; without an image, or with
        ``strength`` >= 1.0, text-to-image (mode rule of StableDiffusionPipeline.Configuration.swift:74-80)."""
        self.check_inputs(prompt, height, width, callback_steps)
        if isinstance(progress_steps, bool) or not isinstance(progress_steps, (int, np.integer)) or progress_steps <= 0:
            raise ValueError(f"`progress_steps` has to be a positive integer but is {progress_steps}")
        if not strength > 0:
            raise ValueError(f"`strength` has to be positive (a fraction of the schedule in (0, 1]) but is {strength}")
        image_to_image = starting_image is not None and strength < 1.0            # Configuration.swift:74-80
        if image_to_image and self.vae_encoder is None:                            # startingImageProvidedWithoutEncoder
            raise ValueError("a starting image needs a VAE encoder: build the pipeline with vae_encoder=...")
        height, width = self.height, self.width
        original_size = original_size or (height, width)
        target_size = target_size or (height, width)
        batch_size = 1 if isinstance(prompt, str) else len(prompt)
        n_img = batch_size * num_images_per_prompt
        do_cfg = guidance_scale > 1.0                                              # pipeline.py:443
        cfg_mul = 2 if do_cfg else 1
        batch_one = bool(unet_batch_one and do_cfg)
        model_batch = self.unet.expected_inputs["sample"]["shape"][0]
        need = 1 if batch_one else cfg_mul * n_img
        if model_batch != need or (batch_one and n_img != 1):
            raise ValueError(
                f"the UNet handle has a static batch of {model_batch} (pipeline.py:112-114) but this call needs {need}: "
                f"{batch_size} prompt(s) x {num_images_per_prompt} image(s) x {cfg_mul} (classifier-free guidance)"
                + (", evaluated one half at a time (--unet-batch-one)" if batch_one else "")
                + f"; build HipModel(batch={need})")

        text_embeddings, pooled = self._encode_prompt(prompt, None, do_cfg, negative_prompt, None)
        text_embeddings = self._per_image(text_embeddings, batch_size, num_images_per_prompt, cfg_mul)
        pooled = self._per_image(pooled, batch_size, num_images_per_prompt, cfg_mul)
        extra = {}
        if self.xl:                                                                # pipeline.py:458-472
            is_refiner = self.unet.expected_inputs["time_ids"]["shape"][-1] == 5   # ...XLPipeline.swift:151-154
            extra = self._xl_kwargs(self.unet, pooled, original_size, crops_coords_top_left, target_size, do_cfg, n_img,
                                    is_refiner)

        if image_to_image:
            latents = self.prepare_image_latents(starting_image, strength, num_inference_steps, n_img, self.unet.in_channels,
                                                 latents, seed, rng)
        else:
            self.scheduler.set_timesteps(num_inference_steps)
            latents = self.prepare_latents(n_img, self.unet.in_channels, height, width, latents, seed, rng)
        timesteps = self.scheduler.timesteps                 # image-to-image: the tail of the schedule (Scheduler.swift:109-114)
        init_latents = latents
        if controlnet_cond:
            controlnet_cond = self.prepare_control_cond(controlnet_cond, do_cfg, batch_size, num_images_per_prompt)
        extra_step_kwargs = self.prepare_extra_step_kwargs(eta)

        # stages: (model, encoder_hidden_states, extra kwargs, [first, last) steps); two when a refiner takes over
        stages = [(self.unet, text_embeddings, extra, 0, len(timesteps))]
        if self.unet_refiner is not None:
            if not self.xl:
                raise ValueError("unet_refiner needs an SDXL pipeline (xl=True)")
            swap = int(float(len(timesteps)) * self.refiner_start)                 # ...XLPipeline.swift:203-206 (truncated count)
            if swap < len(timesteps):
                r_emb, r_pooled = self._encode_prompt(prompt, None, do_cfg, negative_prompt, None, for_refiner=True)
                r_emb = self._per_image(r_emb, batch_size, num_images_per_prompt, cfg_mul)
                r_pooled = self._per_image(r_pooled, batch_size, num_images_per_prompt, cfg_mul)
                r_extra = self._xl_kwargs(self.unet_refiner, r_pooled, original_size, crops_coords_top_left, target_size,
                                          do_cfg, n_img, True)
                stages = [(self.unet, text_embeddings, extra, 0, swap)] if swap > 0 else []
                stages.append((self.unet_refiner, r_emb, r_extra, swap, len(timesteps)))

        reasons = []
        if not device_loop:
            reasons.append("device_loop=False")
        if callback is not None:
            reasons.append("a per-step callback was given")
        if batch_one:
            reasons.append("--unet-batch-one")
        if not hasattr(self.scheduler, "device_tables"):
            reasons.append(f"{type(self.scheduler).__name__} exports no device tables")
        if not all(hasattr(m, "denoise_loop") for m, *_ in stages):
            reasons.append("the UNet model runner has no denoise_loop")
        if controlnet_cond and not (self.controlnet and hasattr(self.unet, "attach_controlnets")
                                    and all(hasattr(cn, "set_controlnet_cond") for cn in self.controlnet)):
            reasons.append("the ControlNet model runners cannot hand residuals over on the device")
        if eta and extra_step_kwargs:
            reasons.append("eta != 0")
        fused = not reasons
        step_ms = None
        cancelled = False
        pred = None
        if progress_handler is not None and use_denoised_intermediates:
            if not hasattr(self.scheduler, "denoised_table"):
                raise NotImplementedError(f"{type(self.scheduler).__name__} exports no de-noised table (use_denoised_intermediates)")
            pred = self.scheduler.denoised_table()

        stopped = []                                        # the handler said stop: kept here, since a stop behind a stage's LAST step
                                                            # leaves as many step times as a full run (denoise_loop's return)

        def report(i, lat_i, den_i):
            """the handler's verdict on step i of the timestep list: True = go on"""
            go = progress_handler(PipelineProgress(self, prompt, i, len(timesteps), den_i if use_denoised_intermediates else lat_i,
                                                   output_type))
            if not (go is None or bool(go)):
                stopped.append(i)
            return not stopped

        if fused:
            if not controlnet_cond and getattr(self.unet, "_attached", None):
                # a previous call attached ControlNets: without conditioning images this call must not run them with the
                # stale ones (the reference would fail on the missing additional_residual_* inputs, pipeline.py:519-529)
                self.unet.attach_controlnets([])
            if controlnet_cond:
                if len(controlnet_cond) != len(self.controlnet):
                    raise ValueError(f"need {len(self.controlnet)} controlnet conditions, got {len(controlnet_cond)}")
                for cn, cond in zip(self.controlnet, controlnet_cond):
                    cn.set_controlnet_cond(cond)
                self.unet.attach_controlnets(self.controlnet)
            ts, coef, hist = self.scheduler.device_tables()
            scale = self.scheduler.sample_scale() if hasattr(self.scheduler, "sample_scale") else None
            lat = latents.astype(np.float32)
            state = np.zeros((hist,) + lat.shape, np.float32) if (hist and len(stages) > 1) else None
            noise = self.scheduler.step_noise(lat.shape) if hasattr(self.scheduler, "step_noise") else None   # ancestral samplers
            step_ms = []
            for model, emb, kw, first, last in stages:
                pkw = {}
                if progress_handler is not None:
                    # `step` runs over both stages; the library thins by the stage's own index, which agrees where the stage starts
                    # on a multiple of progress_steps - else it reports every step and the thinning happens here
                    every = progress_steps if first % progress_steps == 0 else 1
                    pkw = dict(progress_steps=every, pred=None if pred is None else pred[first:last],
                               progress=lambda k, _n, lat_k, den_k, first=first: ((first + k) % progress_steps != 0
                                                                                  or report(first + k, lat_k, den_k)))
                lat, ms = model.denoise_loop(lat, ts[first:last], coef[first:last], guidance_scale, history=hist,
                                             sample_scale=None if scale is None else scale[first:last],
                                             history_state=state, step_noise=None if noise is None else noise[first:last],
                                             encoder_hidden_states=emb.astype(np.float16), **pkw, **kw)
                step_ms.append(ms)
                if stopped:                                  # the handler stopped this stage: a later one does not run
                    cancelled = True
                    break
            latents, step_ms = lat, np.concatenate(step_ms)
        else:
            logger.info("stepping the denoising loop through the host boundary (%s)", "; ".join(reasons))
            if getattr(self.unet, "_attached", None):
                self.unet.attach_controlnets([])           # host-stepped ControlNet residuals travel like the reference's
            if pred is not None:                            # the de-noised estimate on the host: the tap of cfg_sched_step_kernel in numpy
                _, dn_coef, dn_hist = self.scheduler.device_tables()
                m_hist = [np.zeros(latents.shape, np.float32) for _ in range(dn_hist)]
            for i, t in enumerate(timesteps):                                      # pipeline.py:500-573
                model, emb, kw, _, _ = next(s for s in stages if s[3] <= i < s[4])
                x = np.concatenate([latents] * 2) if do_cfg else latents
                x = np.asarray(self.scheduler.scale_model_input(x, t))
                timestep = np.array([t] * (cfg_mul * n_img), np.float16)
                unet_kwargs = dict(kw)
                if controlnet_cond:
                    unet_kwargs.update(self.run_controlnet(x, timestep, emb, controlnet_cond))
                if not batch_one:
                    noise_pred = model(sample=x.astype(np.float16), timestep=timestep,
                                       encoder_hidden_states=emb.astype(np.float16), **unet_kwargs)["noise_pred"]
                    if do_cfg:
                        noise_uncond, noise_text = np.split(noise_pred, 2)
                else:                                                              # pipeline.py:537-556: one half at a time
                    x16, e16, t1 = x.astype(np.float16), emb.astype(np.float16), np.array([t], np.float16)
                    halves = []
                    for h in range(2):
                        kw_h = {k: (v[h:h + 1] if v.shape[0] == 2 else v) for k, v in unet_kwargs.items()}
                        halves.append(model(sample=x16[h:h + 1], timestep=t1, encoder_hidden_states=e16[h:h + 1],
                                            **kw_h)["noise_pred"])
                    noise_uncond, noise_text = halves
                if do_cfg:
                    noise_pred = noise_uncond + guidance_scale * (noise_text - noise_uncond)
                denoised = None
                if pred is not None:
                    x32, out32 = latents.astype(np.float32), np.asarray(noise_pred, np.float32)
                    denoised = pred[i, 0] * x32 + pred[i, 1] * out32
                    for j in range(dn_hist):
                        denoised = denoised + pred[i, 2 + j] * m_hist[j]
                    if dn_hist and dn_coef[i, 7] == 0:      # this step's converted output enters the history behind the tap
                        m_hist = [dn_coef[i, 5] * x32 + dn_coef[i, 6] * out32] + m_hist[:-1]
                latents = self.scheduler.step(noise_pred, t, latents.astype(np.float32), **extra_step_kwargs).prev_sample
                if callback is not None and i % callback_steps == 0:
                    callback(i, t, latents)
                if progress_handler is not None and i % progress_steps == 0:
                    if not report(i, np.array(latents, np.float32), denoised):
                        cancelled = True
                        break

        if cancelled:                                        # Swift returns [] (StableDiffusionPipeline.swift:343-346)
            if not return_dict:
                return [], None
            return PipelineOutput(images=[], nsfw_content_detected=None, step_ms=step_ms, latents=latents, init_latents=init_latents,
                                  cancelled=True)
        if output_type == "latent" or self.vae_decoder is None:
            image, has_nsfw = latents, None                  # the checker looks at images only
        elif self.device_postprocess:
            image, has_nsfw = self.decode_images_on_device(latents, output_type)
        else:
            image = self.decode_latents(latents)
            image, has_nsfw = self.run_safety_checker(image)
        if output_type == "pil" and not isinstance(image, list) and image.ndim == 4 and image.shape[-1] == 3:
            image = self.numpy_to_pil(image)
        if not return_dict:
            return image, has_nsfw
        return PipelineOutput(images=image, nsfw_content_detected=has_nsfw, step_ms=step_ms, latents=latents,
                              init_latents=init_latents, cancelled=False)

    @staticmethod
    def numpy_to_pil(images):
        from PIL import Image
        return [Image.fromarray((im * 255).round().astype("uint8")) for im in images]


class PipelineOutput(SimpleNamespace):
    """``StableDiffusionPipelineOutput`` stand-in: attribute access like diffusers' output class and the
    ``image["images"][0]`` indexing the reference's ``main`` uses (pipeline.py:782)."""

    def __getitem__(self, key):
        return getattr(self, key)


# ---------------------------------------------------------------------------------------------
# get_coreml_pipe / main of the reference over a diffusers checkpoint directory
# ---------------------------------------------------------------------------------------------
def get_available_compute_units():
    """coreml_model.py:205-206 lists Core ML compute units; accepted for CLI compatibility, ignored."""
    return ("ALL", "CPU_AND_GPU", "CPU_ONLY", "CPU_AND_NE")


def _read_json(path):
    with open(path) as f:
        return json.load(f)


def _find_weights(folder):
    for name in ("diffusion_pytorch_model.fp16.safetensors", "diffusion_pytorch_model.safetensors", "model.fp16.safetensors",
                 "model.safetensors"):
        p = os.path.join(folder, name)
        if os.path.exists(p):
            return p
    raise FileNotFoundError(f"no .safetensors checkpoint under {folder} (coreml_model.py:176-178)")


def checkpoint_scheduler_config(model_dir):
    """``pytorch_pipe.scheduler.config`` (pipeline.py:738-741) read from ``scheduler/scheduler_config.json`` of a
    diffusers checkpoint directory; a checkpoint without one gets Stable Diffusion's PNDM config."""
    from .schedulers import load_scheduler_config
    path = os.path.join(model_dir, "scheduler", "scheduler_config.json")
    if os.path.exists(path):
        return load_scheduler_config(path)
    logger.warning("%s not found: assuming Stable Diffusion's PNDM scheduler config", path)
    return load_scheduler_config(dict(_class_name="PNDMScheduler", beta_start=0.00085, beta_end=0.012,
                                      beta_schedule="scaled_linear", skip_prk_steps=True, steps_offset=1))


def get_hip_pipe(model_dir, model_version, compute_unit="ALL", scheduler_override=None, controlnet_models=None,
                 force_zeros_for_empty_prompt=True, sources=None, attention_implementation="SPLIT_EINSUM",
                 num_images=1, guidance_scale=7.5, unet_batch_one=False, latent_size=None, device=0,
                 refiner_dir=None, tokenizer_factory=None, text_encoder_factory=None, vae_dtype=None, disable_safety=False,
                 vae_encoder=False, quantize_nbits=None, palettization_recipe=None, device_postprocess=False,
                 activation_quantization=None, observe_activations=False, unet_weights=None, palette_halo=False):
    """``get_coreml_pipe`` (pipeline.py:607-697) without the conversion step: ``model_dir`` is a diffusers
    checkpoint directory (``unet/``, ``vae/``, ``text_encoder/``, ``tokenizer/``, ``scheduler/`` [,
    ``text_encoder_2/``, ``tokenizer_2/``]) instead of a folder of ``.mlpackage`` files; ControlNets are
    diffusers ControlNet directories.  ``compute_unit`` / ``sources`` are accepted and ignored.  Static shapes
    (pipeline.py:112-114) are fixed here: UNet batch = (2 if guidance_scale > 1 else 1) * num_images.
    ``vae_dtype``: compute precision of the VAE decoder; default = the reference's conversion rule (torch2coreml.py:570-578):
    float32 for an SDXL checkpoint's own VAE (it overflows fp16), float16 otherwise; pass ``np.float16`` for an
    fp16-safe replacement VAE (``--custom-vae-version``).
    ``disable_safety``: do not load ``model_dir/safety_checker/`` (pipeline.py:650-656; ``disableSafety`` of the Swift
    configuration); a checkpoint directory without one runs unchecked either way.
    ``vae_encoder``: also build the VAE encoder from ``vae/`` (image-to-image, ``pipe(..., starting_image=, strength=)``), in the
    decoder's precision; off by default, so a text-to-image pipeline holds no more device memory than before.
    ``quantize_nbits`` (1, 2, 4, 6, 8) / ``palettization_recipe`` ({module: nbits}, ``palettize.load_recipe``): palettize the UNet,
    the refiner UNet and the ControlNets at load time (torch2coreml.py:182-229 ``quantize_weights`` names exactly these models;
    mixed_bit_compression_apply.py); the text encoder, the VAE and the safety checker stay as they are.  A recipe is the UNet's: a
    module of it that the UNet lacks raises ``KeyError``; the ControlNets and the refiner take the modules they share with it (a
    ControlNet has the UNet's down and mid blocks) and leave the rest of their weights fp16.
    ``palette_halo``: those models also keep their palettized 3x3 resnet / upsampler convs palettized on the device (plan tile 25,
    ``Weights.palette_halo``): less memory, the same images; off by default.
    ``device_postprocess``: the 8-bit image and the safety checker's input are made on the device (``HipStableDiffusionPipeline``).
    ``activation_quantization``: a W8A8 recipe, a path or a dict {layer: act_absmax} (``activation_quantization.load_recipe``), applied
    to the UNet alone (activation_quantization.py:141-203 ``--quantize-pytorch``; the refiner and the ControlNets stay as they are;
    parity with coremltools' quantizer unpinned).  ``observe_activations``: the UNet carries the calibration observers
    (``True``, ``"all"``, ``"gemm"``, ``"geglu"``, ``"attn"``, ``"tail"`` or ``"einsum"``: ``Weights.observe_activations``; ``pipe.unet.activation_ranges()`` after a generation;
    ``--calibrate-activations`` / ``--calibrate-scope``).
    ``unet_weights``: a ``Weights`` store the UNet is built from instead of ``unet/``'s checkpoint file; it stays the caller's, who can
    change it and ``reload_weights`` it into ``pipe.unet`` (``mixed_bit_compression_pre_analysis``)."""
    if not os.path.isdir(model_dir):
        raise FileNotFoundError(f"{model_dir} not found (coreml_model.py:176-178)")
    from . import text_encoder as te
    from .hip_model import HipModel, HipVaeDecoder, HipVaeEncoder
    xl = "xl" in model_version
    do_cfg = guidance_scale > 1.0
    batch = 1 if (unet_batch_one and do_cfg) else (2 if do_cfg else 1) * num_images
    if scheduler_override is not None and not isinstance(scheduler_override, str):
        logger.warning("Overriding scheduler in pipeline: Override=%s", type(scheduler_override).__name__)
        scheduler = scheduler_override
    else:
        # pipeline.py:738-741: SCHEDULER_MAP[name].from_config(pytorch_pipe.scheduler.config) - betas, steps_offset,
        # timestep_spacing and prediction_type are the CHECKPOINT's (a v-prediction model with an epsilon scheduler
        # generates garbage); unsupported config values raise instead of being ignored
        sc_cfg = checkpoint_scheduler_config(model_dir)
        name = scheduler_override or sc_cfg["_class_name"].replace("Scheduler", "")
        if name not in SCHEDULER_MAP:
            raise NotImplementedError(f"scheduler {name} is not one of {sorted(SCHEDULER_MAP)}")
        if scheduler_override is not None:
            logger.warning("Overriding scheduler in pipeline: Override=%s", name)
        scheduler = SCHEDULER_MAP[name].from_config(sc_cfg)

    def load_unet(folder, kind="unet", support_controlnet=False, recipe_strict=True, weights=None, **w8a8):
        cfg = dict(_read_json(os.path.join(folder, "config.json")))
        cfg["support_controlnet"] = support_controlnet
        size = latent_size or cfg.get("sample_size", 64)
        return HipModel(cfg, weights if weights is not None else _find_weights(folder), kind=kind, batch=batch, latent_height=size, latent_width=size,
                        attention_implementation=attention_implementation, device=device, quantize_nbits=quantize_nbits,
                        palettization_recipe=palettization_recipe, recipe_strict=recipe_strict, palette_halo=palette_halo, **w8a8)

    kwargs = dict(xl=xl, force_zeros_for_empty_prompt=force_zeros_for_empty_prompt, safety_checker=None)
    logger.info("Loading models in HBM from %s", model_dir)
    kwargs["unet"] = load_unet(os.path.join(model_dir, "unet"), support_controlnet=bool(controlnet_models), weights=unet_weights,
                               activation_quantization=activation_quantization, observe_activations=observe_activations)
    kwargs["controlnet"] = ([load_unet(d, kind="controlnet", recipe_strict=False) for d in controlnet_models] if controlnet_models else None)
    vcfg = _read_json(os.path.join(model_dir, "vae", "config.json"))
    lat = kwargs["unet"].latent_height
    vae_cfg = dict(latent_channels=vcfg.get("latent_channels", 4), out_channels=vcfg.get("out_channels", 3),
                   block_out_channels=tuple(vcfg["block_out_channels"]), layers_per_block=vcfg.get("layers_per_block", 2))
    vae_dtype = np.dtype(vae_dtype) if vae_dtype is not None else np.dtype(np.float32 if xl else np.float16)
    kwargs["vae_decoder"] = HipVaeDecoder(vae_cfg, _find_weights(os.path.join(model_dir, "vae")), batch=1, latent_height=lat,
                                          latent_width=kwargs["unet"].latent_width, device=device, dtype=vae_dtype)
    if vae_encoder:                                                                # Encoder.swift: one starting image, batch 1
        down = 2 ** (len(vae_cfg["block_out_channels"]) - 1)
        kwargs["vae_encoder"] = HipVaeEncoder(vae_cfg, _find_weights(os.path.join(model_dir, "vae")), batch=1, height=lat * down,
                                              width=kwargs["unet"].latent_width * down, device=device, dtype=vae_dtype)
    kwargs["vae_scaling_factor"] = vcfg.get("scaling_factor")
    make_tok = tokenizer_factory or te.load_tokenizer
    make_enc = text_encoder_factory or (lambda folder, **kw: te.HipTextEncoder.from_pretrained(folder, device=device, **kw))
    if xl:
        has_first = os.path.isdir(os.path.join(model_dir, "text_encoder"))       # the refiner ships text_encoder_2 only
        kwargs["tokenizer"] = make_tok(os.path.join(model_dir, "tokenizer")) if has_first else None
        kwargs["text_encoder"] = (make_enc(os.path.join(model_dir, "text_encoder"), xl=True) if has_first else None)
        kwargs["tokenizer_2"] = make_tok(os.path.join(model_dir, "tokenizer_2"))
        kwargs["text_encoder_2"] = make_enc(os.path.join(model_dir, "text_encoder_2"), xl=True)
        if refiner_dir:
            kwargs["unet_refiner"] = load_unet(os.path.join(refiner_dir, "unet"), recipe_strict=False)
    else:
        kwargs["tokenizer"] = make_tok(os.path.join(model_dir, "tokenizer"))
        kwargs["text_encoder"] = make_enc(os.path.join(model_dir, "text_encoder"))
    if not disable_safety and os.path.isdir(os.path.join(model_dir, "safety_checker")):
        from .safety_checker import HipSafetyChecker, load_feature_extractor
        kwargs["feature_extractor"] = load_feature_extractor(os.path.join(model_dir, "feature_extractor"))
        kwargs["safety_checker"] = HipSafetyChecker.from_pretrained(
            os.path.join(model_dir, "safety_checker"), batch=1, device=device,
            image_height=lat * VAE_DECODER_UPSAMPLE_FACTOR, image_width=kwargs["unet"].latent_width * VAE_DECODER_UPSAMPLE_FACTOR)
    logger.info("Initializing HIP pipe for image generation")
    return HipStableDiffusionPipeline(scheduler=scheduler, device_postprocess=device_postprocess, **kwargs)


def get_image_path(args, **override_kwargs):
    """mkdir the output folder and encode metadata in the file name (pipeline.py:700-714)."""
    out_folder = os.path.join(args.o, "_".join(args.prompt.replace("/", "_").rsplit(" ")))
    os.makedirs(out_folder, exist_ok=True)
    out_fname = f"randomSeed_{override_kwargs.get('seed', None) or args.seed}"
    out_fname += f"_computeUnit_{override_kwargs.get('compute_unit', None) or args.compute_unit}"
    out_fname += f"_modelVersion_{override_kwargs.get('model_version', None) or args.model_version.replace('/', '_')}"
    if args.scheduler is not None:
        out_fname += f"_customScheduler_{override_kwargs.get('scheduler', None) or args.scheduler}"
        out_fname += f"_numInferenceSteps{override_kwargs.get('num_inference_steps', None) or args.num_inference_steps}"
    return os.path.join(out_folder, out_fname + ".png")


def prepare_controlnet_cond(image_path, height, width):
    """pipeline.py:717-721: RGB, LANCZOS resize, CHW in [0, 1]."""
    from PIL import Image
    image = Image.open(image_path).convert("RGB")
    image = image.resize((height, width), resample=Image.LANCZOS)
    return np.array(image).transpose(2, 0, 1) / 255.0


def prepare_starting_image(image_path, height, width):
    """The starting image of image-to-image: RGB, LANCZOS resize to the model size, CHW float32 in [-1, 1]
    (``planarRGBShapedArray(minValue: -1, maxValue: 1)``, Encoder.swift:56)."""
    from PIL import Image
    image = Image.open(image_path).convert("RGB")
    image = image.resize((width, height), resample=Image.LANCZOS)
    return (np.array(image).transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)


def build_parser():
    """The reference's flags with their names and defaults (pipeline.py:785-855) plus the run-time
    ``--attention-implementation`` (torch2coreml.py:1678-1685)."""
    parser = argparse.ArgumentParser(prog="python -m python_hip_stable_diffusion.pipeline")
    parser.add_argument("--prompt", required=True, help="The text prompt to be used for text-to-image generation.")
    parser.add_argument("-i", required=True, help="Path to a diffusers checkpoint directory (unet/, vae/, text_encoder/, "
                                                  "tokenizer/, scheduler/); replaces the folder of converted .mlpackage files")
    parser.add_argument("-o", required=True)
    parser.add_argument("--seed", "-s", default=93, type=int, help="Random seed to be able to reproduce results")
    parser.add_argument("--model-version", default="CompVis/stable-diffusion-v1-4",
                        help="The pre-trained model checkpoint and configuration to restore.")
    parser.add_argument("--compute-unit", choices=get_available_compute_units(), default="ALL",
                        help="Accepted for compatibility with the Core ML pipeline and ignored: compute runs on the MI355X.")
    parser.add_argument("--scheduler", choices=tuple(SCHEDULER_MAP.keys()), default=None,
                        help="The scheduler to use for running the reverse diffusion process. If not specified, the "
                             "default scheduler of the checkpoint is utilized.  It is built from the checkpoint's "
                             "scheduler/scheduler_config.json; keys that file omits take the diffusers class defaults, of which "
                             "clip_sample=True (DDIM) and skip_prk_steps=False (PNDM) are not implemented: spell out "
                             "\"clip_sample\": false / \"skip_prk_steps\": true there, as the Stable Diffusion checkpoints do")
    parser.add_argument("--num-inference-steps", default=50, type=int,
                        help="The number of iterations the unet model will be executed throughout the reverse diffusion process")
    parser.add_argument("--guidance-scale", default=7.5, type=float,
                        help="Controls the influence of the text prompt on sampling process (0=random images)")
    parser.add_argument("--controlnet", nargs="*", type=str,
                        help="Enables ControlNet (diffusers ControlNet directories) and the control-UNet inputs. "
                             "For Multi-Controlnet, provide the directories separated by spaces.")
    parser.add_argument("--controlnet-inputs", nargs="*", type=str,
                        help="Image paths for ControlNet inputs, in the order of --controlnet.")
    parser.add_argument("--negative-prompt", default=None,
                        help="The negative text prompt to be used for text-to-image generation.")
    parser.add_argument("--unet-batch-one", action="store_true",
                        help="Do not batch unet predictions for the prompt and negative prompt.")
    parser.add_argument("--model-sources", default=None, choices=["packages", "compiled"],
                        help="Accepted for compatibility and ignored (there is no conversion step).")
    parser.add_argument("--attention-implementation", choices=tuple(_lib.ATTENTION_IMPLEMENTATIONS), default="SPLIT_EINSUM",
                        help="Attention schedule of the UNet kernels (a conversion-time flag in the reference).")
    parser.add_argument("--disable-safety", action="store_true",
                        help="Do not run the checkpoint's safety checker on the generated images (swift CLI --disable-safety).")
    parser.add_argument("--refiner", default=None, help="SDXL: diffusers directory of the refiner checkpoint")
    parser.add_argument("--rng", choices=("numpy", "torch", "nvidia"), default="numpy",
                        help="Seed-exact random source of the initial latents (swift/StableDiffusionCLI/main.swift --rng): "
                             "numpy = np.random.seed + randn (this pipeline's and the reference's default), torch = torch's CPU "
                             "generator, nvidia = torch's CUDA generator (Philox)")
    parser.add_argument("--image", default=None, help="Path to starting image.")          # swift/StableDiffusionCLI/main.swift:45-49
    parser.add_argument("--strength", default=0.5, type=float, help="Strength for image2image.")
    parser.add_argument("--save-every", default=0, type=int,                                      # swift/StableDiffusionCLI/main.swift:57-63
                        help="Save the preview image of every n-th step next to the final image, as <final name>.step<i>.png; "
                             "0 = the final image only")
    parser.add_argument("--device-postprocess", action="store_true",
                        help="Make the 8-bit image and the safety checker's input on the GPU, behind the VAE decoder, instead of in "
                             "numpy / PIL / CLIPImageProcessor on the host; same images and verdicts, bit for bit.")
    parser.add_argument("--quantize-nbits", default=None, choices=(1, 2, 4, 6, 8), type=int,       # torch2coreml.py:1705
                        help="If specified, the UNet / refiner / ControlNet weights are palettized to this many bits at load time "
                             "(k-means LUT per tensor; the conversion-time flag of torch2coreml.py)")
    parser.add_argument("--palette-halo", action="store_true",
                        help="With --quantize-nbits or a recipe: the palettized 3x3 resnet and upsampler convs also stay palettized on the "
                             "GPU (index stream + LUT decoded in the kernel, plan tile 25) instead of being uploaded as fp16; same images, "
                             "less device memory")
    parser.add_argument("--pre-analysis-json-path", default=None,                                # mixed_bit_compression_apply.py
                        help="The JSON file generated by mixed_bit_compression_pre_analysis.py: per-layer palettization recipes")
    parser.add_argument("--selected-recipe", default=None,
                        help="The string key into --pre-analysis-json-path's dict that picks the recipe to apply")
    parser.add_argument("--activation-quantization-recipe", default=None,                        # activation_quantization.py --quantize-pytorch
                        help="A W8A8 recipe (JSON {layer: act_absmax}, written by --calibrate-activations): the UNet convs it names run "
                             "from int8 weights and activations where their kernel is the weight stream, the 3x3 halo conv or - for the plain 1x1 "
                             "projections proj_in / attn1.to_out.0 / attn2.to_out.0 of the 640- and 1280-channel levels - the small-M GEMM, "
                             "or - for their ff.net.0.proj - the GEGLU kernel behind a LayerNorm that writes int8, or - for their attn1.to_q / "
                             "to_k / to_v, all three named with one range - the fused q|k|v launch behind such a LayerNorm, or - for their "
                             "ff.net.2 - the int8-activation GEMM behind the GEGLU, un-merged from proj_out, which then runs on its own")
    parser.add_argument("--calibrate-activations", default=None,                                 # activation_quantization.py --generate-calibration-data
                        help="Run the requested generation on a UNet that records the range of every quantizable conv's input and write "
                             "the W8A8 recipe to this file")
    from .activation_quantization import every_calibration_scope   # CALIBRATION_SCOPES and the scopes added since
    parser.add_argument("--calibrate-scope", default="stream", choices=tuple(every_calibration_scope()),
                        help="Which convs --calibrate-activations observes: 'stream' = those the int8 weight stream takes (the 8x8 level), "
                             "'all' = also every 3x3 / stride-1 conv the int8 halo conv takes, 'gemm' = also the plain 1x1 projections the "
                             "int8 small-M GEMM takes, 'geglu' = also the GEGLU projections ff.net.0.proj the int8 GEGLU kernel takes (the "
                             "output of their norm3), 'attn' = also the self-attention projections attn1.to_q / to_k / to_v the int8 q|k|v "
                             "kernel takes (the output of their norm1: one range under the three names), 'tail' = also ff.net.2 and proj_out of "
                             "the transformer tails the int8-activation GEMM takes (the GEGLU product and ff.net.2's output), 'einsum' = also "
                             "the inputs q, k and v of every self-attention the int8 attention kernel takes (one recipe entry "
                             "<block>.attn1.einsum: [r_q, r_k, r_v])")
    return parser


def main(args):
    """pipeline.py:724-782."""
    logger.info("Setting random seed to %d", args.seed)
    np.random.seed(args.seed)
    scheduler = args.scheduler          # a name: get_hip_pipe builds it from the checkpoint's config (pipeline.py:738-741)
    xl = "xl" in args.model_version
    force_zeros = False                                                            # pipeline.py:744-746
    idx = os.path.join(args.i, "model_index.json")
    if xl and os.path.exists(idx):
        force_zeros = bool(_read_json(idx).get("force_zeros_for_empty_prompt", False))
    recipe = None
    if getattr(args, "pre_analysis_json_path", None) or getattr(args, "selected_recipe", None):
        if not (args.pre_analysis_json_path and args.selected_recipe) or getattr(args, "quantize_nbits", None) is not None:
            raise ValueError("--pre-analysis-json-path and --selected-recipe go together, and not with --quantize-nbits")
        from .palettize import load_recipe
        recipe = load_recipe(args.pre_analysis_json_path, args.selected_recipe)
    palette_halo = bool(getattr(args, "palette_halo", False))
    if palette_halo and getattr(args, "quantize_nbits", None) is None and recipe is None:
        raise ValueError("--palette-halo keeps palettized convs palettized: it goes with --quantize-nbits or --pre-analysis-json-path / --selected-recipe")
    aq_recipe, calibrate = getattr(args, "activation_quantization_recipe", None), getattr(args, "calibrate_activations", None)
    from .activation_quantization import every_calibration_scope
    if aq_recipe and calibrate:
        raise ValueError("--calibrate-activations writes a recipe from the fp16 model; it does not go with --activation-quantization-recipe")
    pipe = get_hip_pipe(args.i, args.model_version, args.compute_unit, scheduler_override=scheduler,
                        controlnet_models=args.controlnet, force_zeros_for_empty_prompt=force_zeros,
                        sources=args.model_sources, attention_implementation=args.attention_implementation,
                        guidance_scale=args.guidance_scale, unet_batch_one=args.unet_batch_one, refiner_dir=args.refiner,
                        disable_safety=getattr(args, "disable_safety", False), vae_encoder=bool(getattr(args, "image", None)),
                        quantize_nbits=getattr(args, "quantize_nbits", None), palettization_recipe=recipe,
                        device_postprocess=getattr(args, "device_postprocess", False), activation_quantization=aq_recipe, palette_halo=palette_halo,
                        observe_activations=every_calibration_scope()[getattr(args, "calibrate_scope", "stream")] if calibrate else False)
    controlnet_cond = None
    if args.controlnet:
        controlnet_cond = [prepare_controlnet_cond(args.controlnet_inputs[i], pipe.height, pipe.width)
                           for i, _ in enumerate(args.controlnet)]
    i2i = {}
    if getattr(args, "image", None):
        i2i = dict(starting_image=prepare_starting_image(args.image, pipe.height, pipe.width), strength=args.strength)
    out_path = get_image_path(args)
    progress = {}
    save_every = getattr(args, "save_every", 0) or 0
    if save_every < 0:
        raise ValueError(f"--save-every has to be 0 or a positive step count but is {save_every}")
    if save_every:                                                                 # StableDiffusionCLI/main.swift:260-263
        stem = os.path.splitext(out_path)[0]

        def save_previews(p):
            logger.info("Step %d of %d", p.step, p.step_count)
            if p.step % save_every == 0:
                p.current_images[0].save(f"{stem}.step{p.step}.png")
            return True

        progress = dict(progress_handler=save_previews)
    logger.info("Beginning image generation.")
    image = pipe(prompt=args.prompt, height=pipe.height, width=pipe.width, num_inference_steps=args.num_inference_steps,
                 guidance_scale=args.guidance_scale, controlnet_cond=controlnet_cond, negative_prompt=args.negative_prompt,
                 unet_batch_one=args.unet_batch_one, seed=args.seed, output_type="pil", rng=getattr(args, "rng", "numpy"), **i2i,
                 **progress)
    logger.info("Saving generated image to %s", out_path)
    image["images"][0].save(out_path)
    if calibrate:
        from . import activation_quantization as aq
        aq.save_recipe(aq.recipe_from_ranges(pipe.unet.activation_ranges()), calibrate)
        logger.info("Saved the activation-quantization recipe to %s", calibrate)
    return out_path


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(build_parser().parse_args())
