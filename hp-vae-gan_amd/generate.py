"""`python -m hp_vae_gan_amd.generate --exp-dir run/<clip>/<checkname>/experiment_<n> --num-samples N`: sample videos
(or images) from a trained experiment; writes samples.npy and one GIF / PNG per sample.

--size T H W (images: H W) samples at another size than the trained one: the generator is fully convolutional and its input is
a noise volume, so every level of the pyramid is drawn at the trained ratio of the requested size (level_sizes).  --wrap AXES
(letters of t, h, w) closes those axes into rings: every convolution of the decoder and the levels sees its input circularly
along them and the resize between levels interpolates across the seam, so a `t` ring is a clip that loops and `hw` a tile.
With either flag the samples go to <exp-dir>/eval/samples_<T>x<H>x<W>[_wrap<axes>] and generate.json is written beside
samples.npy; without them every byte is what it was.

--guide PATH --guide-level N starts the sampling from a given clip (or image) instead of from the decoder's output: the guide goes
through the dataset's own front end at stage N (for the training clip it is bit for bit the trainer's item at that stage) and is
injected as the output of level N (GeneratorHPVAEGAN's sample_init); the levels above re-render it with their noise.  With
--guide-mask hole.npy every sample is kept only inside the hole (dilated and feathered by --guide-feather, ops.mask_blend) and is
the guide, at the finest trained stage, elsewhere: the trained generator's inpainting.  The samples go to
<exp-dir>/eval/samples_guide<N>[_wrap<axes>], with generate.json.  --wrap composes; --size does not."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import checkpoint, datasets, ops
from . import utils as hp_utils
from .modules._nets import Conv
from .programs import (add_guide_flags, check_guide_flags, gpu_device, load_guide_frames, load_opt, networks_of, parse_wrap_axes,
                       pick_mask, refuse_trivial_mask, resume_info, write_samples)


def generate_parser():
    p = argparse.ArgumentParser(prog="python -m hp_vae_gan_amd.generate",
                                description="Sample videos / images from a trained experiment directory.")
    p.add_argument('--exp-dir', required=True, help='experiment_<n> directory of train_video / train_image / '
                   'train_video_baselines')
    p.add_argument('--num-samples', type=int, default=8, help='number of samples')
    p.add_argument('--batch-size', type=int, default=None, help='samples per generator pass (default: the run\'s)')
    p.add_argument('--seed', type=int, default=0, help='seed of the noise')
    p.add_argument('--out', default=None, help='output directory (default: <exp-dir>/eval/samples; with --size / --wrap: '
                   '<exp-dir>/eval/samples_<T>x<H>x<W>[_wrap<axes>])')
    p.add_argument('--size', type=int, nargs='+', default=None, metavar='N',
                   help='finest size T H W (images: H W) to sample at (default: the trained size)')
    p.add_argument('--wrap', default=None, metavar='AXES',
                   help='distinct letters of t, h, w: the axes that are rings (t: a clip that loops; hw: a tile)')
    return add_guide_flags(p)


def level_sizes(trained, size):
    """The shape of every pyramid level for the finest shape `size`, from the trained shapes `trained` (coarsest first, the
    last one the trained finest shape s_L).  Per level and axis, in integers: the trained side where the request equals the
    trained finest side, otherwise max(1, round_half_up(s_l * size / s_L)).  The last level is `size`; size == s_L returns
    `trained` itself."""
    fine = [int(s) for s in trained[-1]]
    size = [int(s) for s in size]
    if len(size) != len(fine):
        raise ValueError("level_sizes: size {} does not fit the trained shape {}".format(size, fine))
    if min(size) < 1:
        raise ValueError("level_sizes: every side must be >= 1, got {}".format(size))
    if size == fine:
        return trained
    return [[int(s[a]) if size[a] == fine[a] else max(1, (2 * int(s[a]) * size[a] + fine[a]) // (2 * fine[a]))
             for a in range(len(fine))] for s in trained]


def check_request(opt, size, wrap):
    """The refusals of --size / --wrap that need no device: host checks on the flags and opt.json.  Returns the ring flags per
    spatial axis of the run (None without --wrap)."""
    image = opt.dims == 2
    if (size is not None or wrap is not None) and getattr(opt, 'program', None) == 'train_video_baselines':
        raise SystemExit("generate: --size / --wrap are not built for a train_video_baselines experiment (its generators pad once "
                         "per stage, not per convolution)")
    if size is not None:
        want = 2 if image else 3
        if len(size) != want:
            raise SystemExit("generate: --size takes {} for this {} run, got {} values".format(
                "H W" if image else "T H W", "image" if image else "video", len(size)))
        if min(size) < 1:
            raise SystemExit("generate: --size: every side must be >= 1, got {}".format(list(size)))
    if wrap is None:
        return None
    flags = parse_wrap_axes(wrap)
    if image and flags[0]:
        raise SystemExit("generate: --wrap t: an image run has no time axis (use letters of h, w)")
    return flags[1:] if image else flags


def check_guide(opt, exp_dir, size, guide, guide_level, guide_mask, guide_feather):
    """The refusals of the --guide flags that need no device: host checks on the flags, opt.json and the files.  Returns None
    without --guide, else a dict: `frames` (the guide trimmed by start_frame / max_frames as the run's input is, host uint8
    [N,H,W,3]), `level`, and with a mask `mask` (host bool, the finest level's (T, H, W)) and `feather`."""
    image = opt.dims == 2
    feather, forms = check_guide_flags("generate", guide, guide_level, guide_mask, guide_feather, image)
    if guide is None:
        return None
    if getattr(opt, 'program', None) == 'train_video_baselines':
        raise SystemExit("generate: --guide is not built for a train_video_baselines experiment (its generators take no "
                         "sample_init)")
    if size is not None:
        raise SystemExit("generate: --guide does not combine with --size: the guide's frame window and size are the trained ones")
    levels = resume_info(os.path.join(exp_dir, 'netG.pth'))[0]   # a host load: the saved generator has this many levels above 0
    if not 0 <= int(guide_level) < levels:
        raise SystemExit("generate: --guide-level must lie in 0 .. {} (the generator has {} levels above the coarsest), got {}".format(
            levels - 1, levels, guide_level))
    frames = load_guide_frames("generate", guide)
    if image:
        frames = frames[:1]
    else:
        start = getattr(opt, "start_frame", 0)
        frames = frames[start:start + opt.max_frames] if getattr(opt, "max_frames", None) else frames[start:]
        need = opt.fps_lcm + 1           # the window of every stage: frames 0, e, 2e, ... fps_lcm
        if len(frames) < need:
            raise SystemExit("generate: --guide has {} frames after --start-frame / --max-frames; the window of level {} needs "
                             "{}".format(len(frames), guide_level, need))
    plan = {"frames": frames, "level": int(guide_level), "mask": None, "feather": feather}
    if forms is not None:
        fine = _stage_shape(opt, levels)
        plan["mask"] = pick_mask(forms, fine, "generate: --guide-mask", "the finest level's")
        refuse_trivial_mask([plan["mask"]], "generate: --guide-mask")
    return plan


def _stage_shape(opt, stage):
    """(T, H, W) of the trainer's item at `stage` (images: T = 1): the level's shape, which is the dataset's."""
    if opt.dims == 3:
        return tuple(hp_utils.images.level_shape_3d(stage, opt))
    return (1,) + tuple(hp_utils.images.level_shape_2d(stage, opt))


def guide_tensors(opt, frames, level, device, finest=None):
    """(x_N, bytes): the guide's frames through the dataset's front end (_DeviceFrames.clip, quantize on, no flip) at stage
    `level` - first frame 0, step sampling_rates[fps index of the stage], the level's frame count and size - as the fp32 tensor
    [3,T,H,W] (images [3,H,W]) the trainer gets at that stage; and, with `finest` (a stage), the same clip at that stage as uint8
    [T,H,W,3] (clip_u8), else None."""
    store = datasets._DeviceFrames(frames, device)

    def window(stage):
        T, H, W = _stage_shape(opt, stage)
        every = opt.sampling_rates[hp_utils.get_fps_td_by_index(stage, opt)[2]] if opt.dims == 3 else 1
        if (T - 1) * every + 1 > store.N:
            raise SystemExit("generate: --guide has {} frames; the window of level {} needs {}".format(store.N, stage, (T - 1) * every + 1))
        return every, T, H, W
    x = store.clip(0, *window(level), False, True)
    return (x if opt.dims == 3 else x[:, 0]), (store.clip_u8(0, *window(finest)) if finest is not None else None)


def load_generator(exp_dir, device):
    """(opt, netG) rebuilt from opt.json, netG.pth and Noise_Amps.pth (weights_only loads; nothing is written back)."""
    opt = load_opt(exp_dir)
    opt.device = device
    netG = getattr(networks_of(opt), opt.generator)(opt)
    scale, amps = checkpoint.resume_generator(netG, exp_dir)
    opt.scale_idx = scale
    opt.Noise_Amps = amps
    return opt, netG.to(device)


def set_ring(netG, ring):
    """Close the axes flagged in `ring` (one 0 / 1 per spatial axis) on the sampling path of a GeneratorHPVAEGAN: every Conv of
    the decoder and the body, and the generator's resize between levels."""
    for part in (netG.decoder, netG.body):
        for m in part.modules():
            if isinstance(m, Conv):
                m.ring = tuple(ring)
    netG.ring = tuple(ring)


def generate(exp_dir, num_samples, batch_size=None, seed=0, out=None, size=None, wrap=None, guide=None, guide_level=None,
             guide_mask=None, guide_feather=None):
    """Draw `num_samples` samples in groups of batch_size (train mode, no_grad: BatchNorm statistics per group, as the
    reference's previews); write samples.npy (uint8 [N, T, H, W, 3], images [N, H, W, 3]) and one GIF / PNG per sample.
    size / wrap / guide*: see the module docstring."""
    ring = check_request(load_opt(exp_dir), size, wrap)   # before the device is asked for
    plan = check_guide(load_opt(exp_dir), exp_dir, size, guide, guide_level, guide_mask, guide_feather)
    flagged = size is not None or wrap is not None or plan is not None
    device = gpu_device()
    opt, netG = load_generator(exp_dir, device)
    bs = int(batch_size or opt.batch_size)
    torch.manual_seed(seed)
    netG.train()
    if opt.dims == 3:
        level0 = hp_utils.images.level_shape_3d(0, opt)
        fps = hp_utils.get_fps_td_by_index(opt.stop_scale, opt)[0]
    else:
        level0 = hp_utils.images.level_shape_2d(0, opt)
        fps = 1
    baseline = getattr(opt, 'program', None) == 'train_video_baselines'
    sizes = None
    if flagged:
        trained = [netG._level_size(l) for l in range(len(netG.body) + 1)]
        sizes = level_sizes(trained, size if size is not None else trained[-1])
        if sizes is not trained:
            netG.level_sizes = sizes
        level0 = sizes[0]
        if ring is not None:
            set_ring(netG, ring)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    size0 = [bs, 3 if baseline else opt.latent_dim, *level0]
    samples = []
    x_guide = guide_u8 = hole = None
    if plan is not None:
        x_guide, guide_u8 = guide_tensors(opt, plan["frames"], plan["level"], device,
                                          len(netG.body) if plan["mask"] is not None else None)
        x_guide = x_guide[None].expand(bs, *x_guide.shape).contiguous()
        if plan["mask"] is not None:
            hole = torch.from_numpy(plan["mask"]).to(device)
    with torch.no_grad(), ops.noise_stream(device):
        if flagged:
            t0.record()
        for _ in range(math.ceil(num_samples / bs)):
            noise_init = hp_utils.generate_noise(size=size0, device=device)
            if baseline:
                fake = netG(noise_init, opt.Noise_Amps, mode='rand')
            elif plan is not None:
                fake, _ = netG(noise_init, opt.Noise_Amps, noise_init=noise_init, sample_init=(plan["level"], x_guide.clone()),
                               mode="rand")
                if hole is not None:
                    u8 = ops.video_to_u8(fake)
                    u8 = u8 if opt.dims == 3 else u8[:, None]
                    u8 = torch.stack([ops.mask_blend(s, guide_u8, hole, plan["feather"]) for s in u8])
                    samples.append((u8 if opt.dims == 3 else u8[:, 0]).cpu().numpy())
                    continue
            else:
                fake, _ = netG(noise_init, opt.Noise_Amps, noise_init=noise_init, mode="rand")
            samples.append(ops.video_to_u8(fake).cpu().numpy())
        if flagged:
            t1.record()
            t1.synchronize()
    arr = np.concatenate(samples, 0)[:num_samples]
    if out is None:
        name = 'samples'
        if flagged:
            name += '_guide{}'.format(plan["level"]) if plan is not None else '_' + 'x'.join(str(int(s)) for s in sizes[-1])
            if wrap is not None:
                name += '_wrap' + wrap
        out = os.path.join(exp_dir, 'eval', name)
    write_samples(out, arr, fps)
    if flagged:
        made = math.ceil(num_samples / bs) * bs
        meta = {"size": [int(s) for s in sizes[-1]], "level_sizes": [[int(s) for s in q] for q in sizes],
                "wrap": wrap, "seed": int(seed), "num_samples": int(num_samples), "batch_size": bs,
                "seconds_per_sample": t0.elapsed_time(t1) / 1000.0 / made}
        if plan is not None:
            meta.update({"guide": os.path.abspath(guide), "guide_level": plan["level"],
                         "guide_mask": os.path.abspath(guide_mask) if guide_mask is not None else None,
                         "guide_feather": list(plan["feather"]) if plan["feather"] is not None else None})
        with open(os.path.join(out, 'generate.json'), 'w') as f:
            json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote {} samples {} to {}".format(len(arr), tuple(arr.shape[1:]), out))
    return arr


def main(argv=None):
    a = generate_parser().parse_args(argv)
    generate(a.exp_dir, a.num_samples, a.batch_size, a.seed, a.out, a.size, a.wrap, a.guide, a.guide_level, a.guide_mask,
             a.guide_feather)
    return 0


if __name__ == "__main__":
    sys.exit(main())
