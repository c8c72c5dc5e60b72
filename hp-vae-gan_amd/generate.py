"""`python -m hp_vae_gan_amd.generate --exp-dir run/<clip>/<checkname>/experiment_<n> --num-samples N`: sample videos
(or images) from a trained experiment; writes samples.npy and one GIF / PNG per sample."""
import argparse
import math
import os
import sys

import numpy as np
import torch

from . import checkpoint, ops
from . import utils as hp_utils
from .programs import gpu_device, load_opt, networks_of, write_samples


def generate_parser():
    p = argparse.ArgumentParser(prog="python -m hp_vae_gan_amd.generate",
                                description="Sample videos / images from a trained experiment directory.")
    p.add_argument('--exp-dir', required=True, help='experiment_<n> directory of train_video / train_image / '
                   'train_video_baselines')
    p.add_argument('--num-samples', type=int, default=8, help='number of samples')
    p.add_argument('--batch-size', type=int, default=None, help='samples per generator pass (default: the run\'s)')
    p.add_argument('--seed', type=int, default=0, help='seed of the noise')
    p.add_argument('--out', default=None, help='output directory (default: <exp-dir>/eval/samples)')
    return p


def load_generator(exp_dir, device):
    """(opt, netG) rebuilt from opt.json, netG.pth and Noise_Amps.pth (weights_only loads; nothing is written back)."""
    opt = load_opt(exp_dir)
    opt.device = device
    netG = getattr(networks_of(opt), opt.generator)(opt)
    scale, amps = checkpoint.resume_generator(netG, exp_dir)
    opt.scale_idx = scale
    opt.Noise_Amps = amps
    return opt, netG.to(device)


def generate(exp_dir, num_samples, batch_size=None, seed=0, out=None):
    """Draw `num_samples` samples in groups of batch_size (train mode, no_grad: BatchNorm statistics per group, as the
    reference's previews); write samples.npy (uint8 [N, T, H, W, 3], images [N, H, W, 3]) and one GIF / PNG per sample."""
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
    size = [bs, 3 if baseline else opt.latent_dim, *level0]
    samples = []
    with torch.no_grad(), ops.noise_stream(device):
        for _ in range(math.ceil(num_samples / bs)):
            noise_init = hp_utils.generate_noise(size=size, device=device)
            if baseline:
                fake = netG(noise_init, opt.Noise_Amps, mode='rand')
            else:
                fake, _ = netG(noise_init, opt.Noise_Amps, noise_init=noise_init, mode="rand")
            samples.append(ops.video_to_u8(fake).cpu().numpy())
    arr = np.concatenate(samples, 0)[:num_samples]
    out = out or os.path.join(exp_dir, 'eval', 'samples')
    write_samples(out, arr, fps)
    print("wrote {} samples {} to {}".format(len(arr), tuple(arr.shape[1:]), out))
    return arr


def main(argv=None):
    a = generate_parser().parse_args(argv)
    generate(a.exp_dir, a.num_samples, a.batch_size, a.seed, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
