"""Shared code of the programs: `python -m hp_vae_gan_amd.train_video`, `.train_image`, `.train_video_baselines` (its own
notes are in train_video_baselines.py), `.generate` and `.evaluate` (scores of the samples against the training clip: exact patch
nearest-neighbour coherence / completeness on the i8 matrix cores, ops.patch_nn, SinGAN's diversity and, with --swd, the exact
sliced Wasserstein distance between the patch distributions, ops.patch_proj_hist / ops.hist_w1).

The trainers follow the reference's programs (train_video.py:265-417, train_image.py:279-440): the same flags, the same
setup (noise_amp_init / scale_factor_init, adjust_scales2image, manualSeed drawn when absent and logged, then random.seed
and torch.manual_seed), DataLoader(shuffle=True, drop_last=True) over a dataset that serves device tensors (so
num_workers=0), and per stage: dataset.generate_frames, the discriminator with its warm-start rule (train_video.py:44-52:
the resume directory on a resumed scale, otherwise the experiment directory), train.train, checkpoint.save_stage.

Run directory: <run-dir>/<clip>/<checkname>/experiment_<n>/ with eval/, numbered as utils/saver.py:23-37 does (one more than
the highest existing number; the reference takes the last of a lexical sort, which only differs from ten experiments on).
<clip> is the input's file name without its extension, or a frame directory's basename.  Beside the checkpoints it holds
opt.json (the parsed flags plus the derived settings `generate` needs; settings only), logbook.txt (every console line),
scalars.jsonl and, with --visualize, previews/.

Scalars: the reference calls .item() on every loss of every iteration (train_video.py:210-222).  Here each iteration
appends its scalars to a device loss log (telemetry.LossLog, captured into the replayed hipGraph) which is drained every
--print-interval iterations and at the end of each stage into scalars.jsonl, one {"tag", "step", "value"} line per value,
under the reference's tags (`Video/Scale {s}/...`, also for images, as train_image.py:227-237 has it) plus
gradient_penalty, total_loss and grad_norm.

Previews (--visualize) at iteration % print_interval == 0, as train_video.py:225-241: real, generated and generated_vae
of that iteration, and 3 x batch_size random draws ("Fake var", "Fake VAE var") made under no_grad with the generator in
train mode (BatchNorm uses batch statistics and updates its running buffers, as in the reference).  Their noise comes from
ops.noise_stream, so it never shares a key with a training draw and no torch or python generator moves: the training
trajectory (weights, optimizer state, losses) is the same with and without previews.  Frames go through
hpvg_video_to_u8_f32 (write_video's conversion) into animated GIFs (video) or PNGs (images).

Resume (--netG <experiment>/netG.pth) follows train_video.py:399-417: the generator grows to the saved scale and loads its
weights and Noise_Amps, and the loop trains the saved scale AGAIN.  Its iteration 0 appends a fresh noise amplitude
(train_video.py:131-145), so Noise_Amps ends one entry longer than the number of scales - the reference's quirk, kept like
the others.  The optimizer state is not restored (neither does the reference).

Not built: mp4 decoding / encoding (cv2), tensorboard event files and neptune (--tag is only recorded), a CPU path
(--no-cuda is refused), multi-GPU launch."""
import argparse
import glob
import json
import math
import os
import random
import sys

import numpy as np
import torch

from . import checkpoint, datasets, ops, telemetry
from . import train as hp_train
from . import utils as hp_utils
from .modules import networks_2d, networks_3d

# column of the loss log -> the reference's scalar tag (train_video.py:210-222) or a tag of its own
TAGS = {"rec_vae_loss": "Rec VAE", "kl_loss": "KLD", "rec_loss": "rec loss", "errG": "errG", "errD_real": "errD_real",
        "errD_fake": "errD_fake", "gradient_penalty": "gradient_penalty", "total_loss": "total_loss", "grad_norm": "grad_norm"}


# ------------------------------------------------------------------------------------------------------------------- flags
def build_parser(kind):
    """The reference's parser of train_video.py (kind 'video') or train_image.py ('image'): same names, types, defaults and
    `required`; plus --run-dir and --no-hip-graph."""
    video = kind == "video"
    p = argparse.ArgumentParser(prog="python -m hp_vae_gan_amd.train_" + kind,
                                description="Train HP-VAE-GAN on one %s, stage by stage, on an MI355X." % kind)
    a = p.add_argument
    # load, input, save
    a('--netG', default='', help='netG.pth of an experiment to resume from (its scale is trained again)')
    a('--netD', default='', help='accepted, unused (as in the reference)')
    a('--manualSeed', type=int, help='seed of python random and torch (random when absent)')
    # networks
    a('--nc-im', type=int, default=3, help='image channels')
    a('--nfc', type=int, default=64, help='base channel count')
    a('--latent-dim', type=int, default=128, help='VAE latent channels')
    a('--vae-levels', type=int, default=3, help='number of VAE levels')
    a('--enc-blocks', type=int, default=2, help='encoder blocks')
    a('--ker-size', type=int, default=3, help='kernel size')
    a('--num-layer', type=int, default=5, help='layers per block')
    a('--stride', default=1, help='stride')
    a('--padd-size', type=int, default=1, help='padding')
    a('--generator', type=str, default='GeneratorHPVAEGAN', help='generator class')
    a('--discriminator', type=str, default='WDiscriminator3D' if video else 'WDiscriminator2D', help='discriminator class')
    # pyramid
    a('--scale-factor', type=float, default=0.75, help='pyramid scale factor')
    a('--noise_amp', type=float, default=0.1, help='additive noise weight')
    a('--min-size', type=int, default=32, help='size of the coarsest scale')
    a('--max-size', type=int, default=256, help='size of the finest scale')
    # optimisation
    a('--niter', type=int, default=50000, help='iterations per scale')
    a('--lr-g', type=float, default=0.0005, help='generator learning rate')
    a('--lr-d', type=float, default=0.0005, help='discriminator learning rate')
    a('--beta1', type=float, default=0.5, help='Adam beta1')
    a('--lambda-grad', type=float, default=0.1, help='gradient penalty weight')
    a('--rec-weight', type=float, default=10., help='reconstruction loss weight')
    a('--kl-weight', type=float, default=1., help='KL weight')
    a('--disc-loss-weight', type=float, default=1.0, help='adversarial loss weight')
    a('--lr-scale', type=float, default=0.2, help='learning-rate scaling of the lower trained levels')
    a('--train-depth', type=int, default=1, help='levels trained at once')
    a('--grad-clip', type=float, default=5, help='gradient clip norm')
    a('--const-amp', action='store_true', default=False, help='constant noise amplitude')
    a('--train-all', action='store_true', default=False, help='train all levels w.r.t. train-depth')
    # data
    if video:
        a('--video-path', required=True, help='frame directory or .npy [N,H,W,3] uint8 (no mp4 decoder in this build)')
        a('--start-frame', default=0, type=int, help='first frame')
        a('--max-frames', default=1000, type=int, help='frames to keep')
    else:
        a('--image-path', required=True, help='image file, directory of images or .npy [N,H,W,3] uint8')
    a('--hflip', action='store_true', default=False, help='random horizontal flips')
    a('--img-size', type=int, default=256)
    if video:
        a('--sampling-rates', type=int, nargs='+', default=[4, 3, 2, 1], help='temporal sampling rates')
    a('--stop-scale-time', type=int, default=-1)
    a('--data-rep', type=int, default=1 if video else 1000, help='dataset repetitions')
    # main
    a('--checkname', type=str, default='DEBUG', help='run name')
    a('--mode', default='train', help='task')
    a('--batch-size', type=int, default=2, help='batch size')
    a('--print-interval', type=int, default=100, help='iterations between log drains (and previews)')
    a('--visualize', action='store_true', default=False, help='write previews (GIF / PNG) under previews/')
    a('--no-cuda', action='store_true', default=False, help='refused: there is no CPU path')
    if not video:
        a('--tag', type=str, default='', help='recorded in opt.json only (the reference tags a neptune run)')
    # this project's own
    a('--run-dir', default='run', help='root of the run directories')
    a('--no-hip-graph', action='store_true', default=False, help='stay eager (no hipGraph replay)')
    p.set_defaults(hflip=False)
    return p


# ---------------------------------------------------------------------------------------------------------- run directory
def clip_name(path):
    """<clip> of the run directory: the file name without its extension (utils/saver.py:26), a directory's basename."""
    path = os.path.normpath(path)
    base = os.path.basename(path)
    if os.path.isdir(path) or '.' not in base:
        return base
    return '.'.join(base.split('.')[:-1])


def experiment_dir(run_dir, clip, checkname):
    """Create and return <run_dir>/<clip>/<checkname>/experiment_<n> (and its eval/): n = 1 + the highest existing number."""
    directory = os.path.join(run_dir, clip, checkname)
    nums = []
    for d in glob.glob(os.path.join(directory, 'experiment_*')):
        tail = d.rsplit('_', 1)[-1]
        if tail.isdigit():
            nums.append(int(tail))
    exp = os.path.join(directory, 'experiment_{}'.format(max(nums) + 1 if nums else 0))
    os.makedirs(os.path.join(exp, 'eval'), exist_ok=True)
    return exp


def resume_info(netG_path):
    """(scale, resume_dir) of a --netG checkpoint (train_video.py:399-403)."""
    if not os.path.isfile(netG_path):
        raise RuntimeError("=> no <G> checkpoint found at '{}'".format(netG_path))
    ckpt = torch.load(netG_path, map_location='cpu', weights_only=True)
    return int(ckpt['scale']), os.path.dirname(netG_path)


def stage_plan(scale_idx, resumed_idx, stop_scale):
    """[(scale, grow the generator first?)] of the stage loop (train_video.py:413-417): a fresh run grows at every scale
    above 0; a resumed run starts at the saved scale without growing (the checkpoint already holds that level)."""
    return [(s, s > 0 and s != resumed_idx) for s in range(scale_idx, stop_scale + 1)]


def json_settings(opt):
    """The JSON-representable settings of `opt` (no tensors, devices, datasets or code)."""
    out = {}
    for k, v in sorted(vars(opt).items()):
        if isinstance(v, (bool, int, float, str)) or v is None:
            out[k] = v
        elif isinstance(v, (list, tuple)) and all(isinstance(e, (bool, int, float, str)) for e in v):
            out[k] = list(v)
    return out


class Logbook:
    """print() to the console and to <experiment>/logbook.txt."""

    def __init__(self, path):
        self.f = open(path, 'a')

    def __call__(self, msg):
        print(msg, flush=True)
        self.f.write(msg + '\n')
        self.f.flush()

    def close(self):
        self.f.close()


# --------------------------------------------------------------------------------------------------------- frames on disk
def write_frames(u8, path, fps):
    """u8: [T][H][W][C] or [H][W][C] uint8 -> an animated GIF (video) or a PNG (image)."""
    from PIL import Image
    if u8.shape[-1] == 1:
        u8 = u8[..., 0]
    if path.endswith('.gif'):
        frames = [Image.fromarray(f) for f in u8]
        frames[0].save(path, save_all=True, append_images=frames[1:], duration=max(1, int(round(1000.0 / fps))), loop=0)
    else:
        Image.fromarray(u8).save(path)


# ------------------------------------------------------------------------------------------------------------ training
def _networks(opt):
    return networks_3d if opt.dims == 3 else networks_2d


def _stage_data(loader, holder):
    """Iterate the DataLoader and remember the batch at hand (the previews show `real`)."""
    for item in loader:
        holder[0] = item
        yield item


class _Stage:
    """Callback of train.train for one stage: drains the loss log into scalars.jsonl, prints progress, writes previews."""

    def __init__(self, prog, trainer_log, holder):
        self.prog, self.log, self.holder = prog, trainer_log, holder

    def __call__(self, trainer, out):
        opt = self.prog.opt
        i = trainer.iteration - 1
        if opt.visualize and i % opt.print_interval == 0:
            self.prog.preview(trainer, out, self.holder[0], i)
        if trainer.iteration % opt.print_interval == 0:
            self.prog.drain(self.log)


class Program:
    """One training run of train_video / train_image (see the module docstring)."""

    tags = TAGS   # loss-log column -> scalar tag

    def logs_noise_amp(self):
        return True

    def __init__(self, kind, argv=None):
        self.kind = kind
        opt = build_parser(kind).parse_args(argv)
        if opt.no_cuda:
            raise SystemExit("--no-cuda: hp-vae-gan_amd has no CPU path; every op runs on an MI355X")
        self.path = opt.video_path if kind == 'video' else opt.image_path
        if self.path.lower().endswith('.mp4') or not os.path.exists(self.path):
            datasets.load_frames(self.path)   # the data front-end's own error (no decoder / missing file)
        if not torch.cuda.is_available():
            raise SystemExit("hp-vae-gan_amd: no GPU visible; every op runs on an MI355X")
        assert opt.vae_levels > 0
        assert opt.disc_loss_weight > 0
        if kind == 'image' and opt.data_rep < opt.batch_size:
            opt.data_rep = opt.batch_size
        opt.dims = 3 if kind == 'video' else 2
        opt.hip_graph = not opt.no_hip_graph
        self.exp_dir = experiment_dir(opt.run_dir, clip_name(self.path), opt.checkname)
        opt.experiment_dir = self.exp_dir
        self.log = Logbook(os.path.join(self.exp_dir, 'logbook.txt'))
        self.scalars = open(os.path.join(self.exp_dir, 'scalars.jsonl'), 'a')
        opt.device = torch.device('cuda', torch.cuda.current_device())
        opt.noise_amp_init = opt.noise_amp
        opt.scale_factor_init = opt.scale_factor
        hp_utils.adjust_scales2image(opt.img_size, opt)
        if opt.manualSeed is None:
            opt.manualSeed = random.randint(1, 10000)
        self.log("Random Seed: {}".format(opt.manualSeed))
        random.seed(opt.manualSeed)
        torch.manual_seed(opt.manualSeed)
        opt.scale_idx = 0
        opt.nfc_prev = 0
        opt.Noise_Amps = []
        if kind == 'video':
            self.dataset = datasets.SingleVideoDataset(opt)
        else:
            self.dataset = datasets.SingleImageDataset(opt)
        self.loader = torch.utils.data.DataLoader(self.dataset, shuffle=True, drop_last=True, batch_size=opt.batch_size,
                                                  num_workers=0)
        if opt.stop_scale_time == -1:
            opt.stop_scale_time = opt.stop_scale
        self.opt = opt
        with open(os.path.join(self.exp_dir, 'opt.json'), 'w') as f:
            json.dump(json_settings(opt), f, indent=1, sort_keys=True)
        for k, v in json_settings(opt).items():
            self.log('{}: {}'.format(k, v))
        self.log("Experiment: {}".format(self.exp_dir))
        self.netG = getattr(_networks(opt), opt.generator)(opt).to(opt.device)
        if opt.netG != '':
            opt.scale_idx, opt.resume_dir = resume_info(opt.netG)
            opt.resumed_idx = opt.scale_idx
            _, opt.Noise_Amps = checkpoint.resume_generator(self.netG, opt.resume_dir)
            self.netG.to(opt.device)
            self.log("Resumed scale {} from {} (Noise_Amps {})".format(opt.scale_idx, opt.resume_dir, opt.Noise_Amps))
        else:
            opt.resumed_idx = -1
        self.trainers = []
        self.logs = []

    # ---- one stage
    def make_discriminator(self):
        opt = self.opt
        if not opt.vae_levels < opt.scale_idx + 1:
            return None
        netD = getattr(_networks(opt), opt.discriminator)(opt).to(opt.device)
        if opt.netG != '' and opt.resumed_idx == opt.scale_idx:
            checkpoint.warm_start_discriminator(netD, opt.resume_dir, opt.scale_idx)
        elif opt.vae_levels < opt.scale_idx:
            checkpoint.warm_start_discriminator(netD, self.exp_dir, opt.scale_idx)
        return netD

    def train_stage(self):
        opt = self.opt
        if opt.dims == 3:
            opt.fps, opt.td, opt.fps_index = hp_utils.get_fps_td_by_index(opt.scale_idx, opt)
            self.log("Scale {}: FPS {}, time depth {}, sampling rate {}".format(
                opt.scale_idx, opt.fps, opt.td, opt.sampling_rates[opt.fps_index]))
            self.dataset.generate_frames(opt.scale_idx)
        netD = self.make_discriminator()
        is_gan = netD is not None
        log = telemetry.LossLog(hp_train.loss_log_columns(is_gan), capacity=max(64, 2 * opt.print_interval),
                                device=opt.device)
        holder = [None]
        trainer = hp_train.train(opt, self.netG, _Loop(self.loader, holder), netD=netD, loss_log=log,
                                 callback=_Stage(self, log, holder))
        if trainer.iteration % opt.print_interval != 0:
            self.drain(log)
        checkpoint.save_stage(self.exp_dir, opt, trainer)
        self.trainers.append(trainer)
        self.logs.append(log)
        return trainer

    def run(self):
        opt = self.opt
        for scale, grow in stage_plan(opt.scale_idx, opt.resumed_idx, opt.stop_scale):
            opt.scale_idx = scale
            if grow:
                self.netG.init_next_stage()
                self.netG.to(opt.device)
            self.train_stage()
        opt.scale_idx = opt.stop_scale + 1
        torch.cuda.synchronize()
        self.log("Done: {}".format(self.exp_dir))
        self.scalars.close()
        self.log.close()
        return self

    # ---- scalars
    def drain(self, log):
        opt = self.opt
        idx, rows, lost = log.drain()
        if lost:
            self.log("Scale {}: the loss log lost {} rows before this drain".format(opt.scale_idx, lost))
        prefix = 'Video/Scale {}/'.format(opt.scale_idx)
        tags = self.tags
        for step, row in zip(idx.tolist(), rows):
            lines = [{"tag": prefix + "noise_amp", "step": step, "value": float(opt.noise_amp)}] if self.logs_noise_amp() else []
            lines += [{"tag": prefix + tags[c], "step": step, "value": float(v)} for c, v in zip(log.columns, row)]
            for ln in lines:
                self.scalars.write(json.dumps(ln) + '\n')
        self.scalars.flush()
        if len(idx):
            last = ', '.join('{} {:.5g}'.format(tags[c], float(v)) for c, v in zip(log.columns, rows[-1]))
            self.log('Scale [{}/{}], Iteration [{}/{}]: noise_amp {:.5g}, {}'.format(
                opt.scale_idx + 1, opt.stop_scale + 1, int(idx[-1]) + 1, opt.niter, float(opt.noise_amp), last))

    # ---- previews
    def sample(self, count=3):
        """`count` rand draws of batch_size from the current generator (train mode, no_grad, ops.noise_stream):
        (fake, fake_vae), each [count * batch_size, C, ...]."""
        opt, netG = self.opt, self.netG
        fakes, vaes = [], []
        with torch.no_grad(), ops.noise_stream(opt.device):
            for _ in range(count):
                noise_init = hp_utils.generate_noise(size=opt.Z_init_size, device=opt.device)
                fake, fake_vae = netG(noise_init, opt.Noise_Amps, noise_init=noise_init, mode="rand")
                fakes.append(fake)
                vaes.append(fake_vae)
        return torch.cat(fakes, 0), torch.cat(vaes, 0)

    def preview(self, trainer, out, batch, iteration):
        opt = self.opt
        real = batch[0] if isinstance(batch, (list, tuple)) else batch
        fake_var, fake_vae_var = self.sample()
        d = os.path.join(self.exp_dir, 'previews')
        os.makedirs(d, exist_ok=True)
        ext = '.gif' if opt.dims == 3 else '.png'
        fps = getattr(opt, 'fps', 1)
        for name, x in (('real', real), ('generated', out['generated']), ('generated_vae', out['generated_vae']),
                        ('fake_var', fake_var), ('fake_vae_var', fake_vae_var)):
            u8 = ops.video_to_u8(x.float()).cpu().numpy()
            for b in range(u8.shape[0]):
                write_frames(u8[b], os.path.join(d, 'scale{}_iter{:06d}_{}_{}{}'.format(opt.scale_idx, iteration, name, b, ext)),
                             fps)


class _Loop:
    """Re-iterable view of the DataLoader that remembers the batch at hand (train.train restarts an exhausted iterator)."""

    def __init__(self, loader, holder):
        self.loader, self.holder = loader, holder

    def __iter__(self):
        return _stage_data(self.loader, self.holder)


def train_main(kind, argv=None):
    Program(kind, argv).run()
    return 0


# ------------------------------------------------------------------------------------------------ train_video_baselines
# column of the baselines' loss log -> the reference's tag (train_video_baselines.py:178-184: `rec_loss`, not train_video's
# `rec loss`) or this project's own (gradient_penalty)
BASELINE_TAGS = {"errD_real": "errD_real", "errD_fake": "errD_fake", "gradient_penalty": "gradient_penalty", "errG": "errG",
                 "rec_loss": "rec_loss"}


def build_baseline_parser():
    """The reference's parser of train_video_baselines.py:217-272 (same names, types, defaults and `required`), plus --run-dir
    and --no-hip-graph."""
    p = argparse.ArgumentParser(prog="python -m hp_vae_gan_amd.train_video_baselines",
                                description="Train a SinGAN-3D baseline on one video, stage by stage, on an MI355X.")
    a = p.add_argument
    # load, input, save
    a('--netG', default='', help='netG.pth of an experiment to resume from (its scale is trained again)')
    a('--netD', default='', help='accepted, unused (as in the reference)')
    a('--manualSeed', type=int, help='seed of python random and torch (random when absent)')
    # networks
    a('--nc-z', type=int, default=3, help='noise channels')
    a('--nc-im', type=int, help='image channels', default=3)
    a('--nfc', type=int, default=64, help='base channel count')
    a('--ker-size', type=int, default=3, help='kernel size')
    a('--num-layer', type=int, default=5, help='layers per stage')
    a('--stride', default=1, help='stride')
    a('--padd-size', type=int, default=1, help='padding of the critic convolutions')
    a('--generator', type=str, help='generator class (GeneratorCSG, GeneratorSG)', default='GeneratorCSG')
    a('--discriminator', type=str, help='discriminator class (WDiscriminator3D, WDiscriminatorBaselines)',
      default='WDiscriminator3D')
    # pyramid
    a('--scale-factor', type=float, default=0.75, help='pyramid scale factor')
    a('--noise_amp', type=float, default=0.1, help='additive noise weight')
    a('--min-size', type=int, default=32, help='size of the coarsest scale')
    a('--max-size', type=int, default=256, help='size of the finest scale')
    # optimisation
    a('--niter', type=int, default=50000, help='iterations per scale')
    a('--lr-g', type=float, default=0.0005, help='generator learning rate')
    a('--lr-d', type=float, default=0.0005, help='discriminator learning rate')
    a('--beta1', type=float, default=0.5, help='Adam beta1')
    a('--disc-loss-weight', type=float, default=1.0, help='adversarial loss weight')
    a('--Gsteps', type=int, default=1, help='generator optimizer steps per iteration')
    a('--Dsteps', type=int, default=1, help='discriminator updates per iteration')
    a('--lambda-grad', type=float, default=0.1, help='gradient penalty weight')
    a('--alpha', type=float, help='reconstruction loss weight', default=10.)
    a('--lr-scale', type=float, default=0.2, help='learning-rate scaling of the lower trained stages')
    a('--train-depth', type=int, default=1, help='stages trained at once')
    # data
    a('--video-path', required=True, help='frame directory or .npy [N,H,W,3] uint8 (no mp4 decoder in this build)')
    a('--start-frame', default=0, type=int, help='first frame')
    a('--max-frames', default=1000, type=int, help='frames to keep')
    a('--hflip', action='store_true', default=False, help='random horizontal flips')
    a('--img-size', type=int, default=256)
    a('--sampling-rates', type=int, nargs='+', default=[4, 3, 2, 1], help='temporal sampling rates')
    a('--stop-scale-time', type=int, default=-1)
    a('--data-rep', type=int, default=1, help='dataset repetitions')
    # main
    a('--checkname', type=str, default='DEBUG', help='run name')
    a('--mode', default='train', help='accepted, unused (as in the reference)')
    a('--batch-size', type=int, default=2, help='batch size')
    a('--print-interval', type=int, default=100, help='iterations between log drains (and previews)')
    a('--visualize', action='store_true', default=False, help='write GIF previews under previews/')
    a('--no-cuda', action='store_true', default=False, help='refused: there is no CPU path')
    # this project's own
    a('--run-dir', default='run', help='root of the run directories')
    a('--no-hip-graph', action='store_true', default=False, help='stay eager (no hipGraph replay)')
    p.set_defaults(hflip=False)
    return p


def z_init_shape(opt):
    """Shape of the baselines' fixed reconstruction noise (train_video_baselines.py:38-43): [B, 3, opt.td, H0, W0] with the
    level-0 width and height and the time depth of the stage being trained when it is drawn (the first one of the process)."""
    w = hp_utils.get_scales_by_index(0, opt.scale_factor, opt.stop_scale, opt.img_size)
    return [opt.batch_size, 3, opt.td, int(w * opt.ar), w]


def baseline_netD_dir(opt, exp_dir):
    """Directory whose netD_{s-1}.pth warm-starts the critic of stage s = opt.scale_idx, or None at stage 0.  On the resumed
    scale that is the resume directory; the reference reads its experiment directory there too (train_video_baselines.py:45-48),
    which holds no such file after a resume."""
    if opt.scale_idx == 0:
        return None
    if opt.netG != '' and opt.resumed_idx == opt.scale_idx:
        return opt.resume_dir
    return exp_dir


class BaselineProgram(Program):
    """One training run of train_video_baselines (see the module docstring of train_video_baselines.py)."""

    tags = BASELINE_TAGS

    def __init__(self, argv=None):
        self.kind = 'video'
        opt = build_baseline_parser().parse_args(argv)
        if opt.no_cuda:
            raise SystemExit("--no-cuda: hp-vae-gan_amd has no CPU path; every op runs on an MI355X")
        self.path = opt.video_path
        if self.path.lower().endswith('.mp4') or not os.path.exists(self.path):
            datasets.load_frames(self.path)   # the data front-end's own error (no decoder / missing file)
        if not torch.cuda.is_available():
            raise SystemExit("hp-vae-gan_amd: no GPU visible; every op runs on an MI355X")
        assert opt.disc_loss_weight > 0
        opt.program = 'train_video_baselines'
        opt.dims = 3
        opt.hip_graph = not opt.no_hip_graph
        self.exp_dir = experiment_dir(opt.run_dir, clip_name(self.path), opt.checkname)
        opt.experiment_dir = self.exp_dir
        self.log = Logbook(os.path.join(self.exp_dir, 'logbook.txt'))
        self.scalars = open(os.path.join(self.exp_dir, 'scalars.jsonl'), 'a')
        opt.device = torch.device('cuda', torch.cuda.current_device())
        opt.noise_amp_init = opt.noise_amp
        opt.scale_factor_init = opt.scale_factor
        hp_utils.adjust_scales2image(opt.img_size, opt)
        if opt.manualSeed is None:
            opt.manualSeed = random.randint(1, 10000)
        self.log("Random Seed: {}".format(opt.manualSeed))
        random.seed(opt.manualSeed)
        torch.manual_seed(opt.manualSeed)
        opt.scale_idx = 0
        opt.nfc_prev = 0
        opt.Noise_Amps = []
        self.dataset = datasets.SingleVideoDataset(opt)
        self.loader = torch.utils.data.DataLoader(self.dataset, shuffle=True, drop_last=True, batch_size=opt.batch_size,
                                                  num_workers=0)
        if opt.stop_scale_time == -1:
            opt.stop_scale_time = opt.stop_scale
        self.opt = opt
        with open(os.path.join(self.exp_dir, 'opt.json'), 'w') as f:
            json.dump(json_settings(opt), f, indent=1, sort_keys=True)
        for k, v in json_settings(opt).items():
            self.log('{}: {}'.format(k, v))
        opt.Z_init = None   # drawn at the first stage this process trains
        self.log("Experiment: {}".format(self.exp_dir))
        self.netG = getattr(networks_3d, opt.generator)(opt).to(opt.device)
        if opt.netG != '':
            opt.scale_idx, opt.resume_dir = resume_info(opt.netG)
            opt.resumed_idx = opt.scale_idx
            _, opt.Noise_Amps = checkpoint.resume_generator(self.netG, opt.resume_dir)
            self.netG.to(opt.device)
            self.log("Resumed scale {} from {} (Noise_Amps {})".format(opt.scale_idx, opt.resume_dir, opt.Noise_Amps))
        else:
            opt.resumed_idx = -1
        self.trainers = []
        self.logs = []

    def logs_noise_amp(self):
        return self.opt.alpha > 0   # (train_video_baselines.py:181-184)

    def save_z_init(self):
        torch.save({'data': self.opt.Z_init.detach().cpu()}, os.path.join(self.exp_dir, 'Z_init.pth'))

    def train_stage(self):
        opt = self.opt
        opt.fps, opt.td, opt.fps_index = hp_utils.get_fps_td_by_index(opt.scale_idx, opt)
        self.log("Scale {}: FPS {}, time depth {}, sampling rate {}".format(
            opt.scale_idx, opt.fps, opt.td, opt.sampling_rates[opt.fps_index]))
        self.dataset.generate_frames(opt.scale_idx)
        if opt.Z_init is None:
            opt.Z_init = hp_utils.generate_noise(size=z_init_shape(opt), device=opt.device)
            self.save_z_init()
        netD = getattr(networks_3d, opt.discriminator)(opt).to(opt.device)
        src = baseline_netD_dir(opt, self.exp_dir)
        if src is not None:
            checkpoint.warm_start_discriminator(netD, src, opt.scale_idx)
            self.log("Scale {}: critic warm-started from {}".format(opt.scale_idx,
                                                                   os.path.join(src, 'netD_{}.pth'.format(opt.scale_idx - 1))))
        log = telemetry.LossLog(hp_train.baseline_loss_log_columns(opt.alpha), capacity=max(64, 2 * opt.print_interval),
                                device=opt.device)
        holder = [None]
        trainer = hp_train.train_baseline(opt, self.netG, _Loop(self.loader, holder), netD=netD, loss_log=log,
                                          callback=_Stage(self, log, holder))
        if trainer.iteration % opt.print_interval != 0:
            self.drain(log)
        self.log("Scale {}: {} iterations, hipGraph replay {}".format(
            opt.scale_idx, trainer.iteration, 'on' if getattr(trainer, '_graph', None) is not None else 'off'))
        self.save_z_init()
        checkpoint.save_stage(self.exp_dir, opt, trainer)
        self.trainers.append(trainer)
        self.logs.append(log)
        return trainer

    def preview(self, trainer, out, batch, iteration):
        """real, generated (alpha > 0) and fake of this iteration (train_video_baselines.py:190-196); no extra draws."""
        opt = self.opt
        real = batch[0] if isinstance(batch, (list, tuple)) else batch
        d = os.path.join(self.exp_dir, 'previews')
        os.makedirs(d, exist_ok=True)
        for name, x in (('real', real), ('generated', out['generated']), ('fake', out['fake'])):
            if x is None:
                continue
            u8 = ops.video_to_u8(x.float()).cpu().numpy()
            for b in range(u8.shape[0]):
                write_frames(u8[b], os.path.join(d, 'scale{}_iter{:06d}_{}_{}.gif'.format(opt.scale_idx, iteration, name, b)),
                             opt.fps)


def baseline_main(argv=None):
    BaselineProgram(argv).run()
    return 0


# ------------------------------------------------------------------------------------------------------------ generate
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
    import types
    with open(os.path.join(exp_dir, 'opt.json')) as f:
        opt = types.SimpleNamespace(**json.load(f))
    opt.device = device
    netG = getattr(_networks(opt), opt.generator)(opt)
    scale, amps = checkpoint.resume_generator(netG, exp_dir)
    opt.scale_idx = scale
    opt.Noise_Amps = amps
    return opt, netG.to(device)


def generate(exp_dir, num_samples, batch_size=None, seed=0, out=None):
    """Draw `num_samples` samples in groups of batch_size (train mode, no_grad: BatchNorm statistics per group, as the
    reference's previews); write samples.npy (uint8 [N, T, H, W, 3], images [N, H, W, 3]) and one GIF / PNG per sample."""
    if not torch.cuda.is_available():
        raise SystemExit("hp-vae-gan_amd: no GPU visible; every op runs on an MI355X")
    device = torch.device('cuda', torch.cuda.current_device())
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
    os.makedirs(out, exist_ok=True)
    np.save(os.path.join(out, 'samples.npy'), arr)
    ext = '.gif' if opt.dims == 3 else '.png'
    for i, a in enumerate(arr):
        write_frames(a, os.path.join(out, 'sample_{:04d}{}'.format(i, ext)), fps)
    print("wrote {} samples {} to {}".format(len(arr), tuple(arr.shape[1:]), out))
    return arr


def generate_main(argv=None):
    a = generate_parser().parse_args(argv)
    generate(a.exp_dir, a.num_samples, a.batch_size, a.seed, a.out)
    return 0


# ------------------------------------------------------------------------------------------------------------ evaluate
def evaluate_parser():
    p = argparse.ArgumentParser(prog="python -m hp_vae_gan_amd.evaluate",
                                description="Score samples against the training clip: exact patch nearest-neighbour "
                                "coherence / completeness (bidirectional similarity) and SinGAN's diversity.")
    p.add_argument('--exp-dir', default=None, help='experiment_<n> directory (gives the samples\' default place and the real volume)')
    p.add_argument('--samples', default=None, help='samples.npy, uint8 [N,T,H,W,3] or [N,H,W,3] (default: <exp-dir>/eval/samples/'
                   'samples.npy, as `generate` writes it)')
    p.add_argument('--real', default=None, help='the real clip / image (.npy, frame directory or image file); with --exp-dir it '
                   'replaces the run\'s input and is trimmed, sampled and resized like it; without, it is used as it is')
    p.add_argument('--patch', type=int, nargs=3, default=None, metavar=('T', 'H', 'W'), help='patch (default 3 7 7, images 1 7 7)')
    p.add_argument('--stride', type=int, nargs=3, default=[1, 1, 1], metavar=('T', 'H', 'W'),
                   help='stride of the query side of each direction (the other side is always dense)')
    p.add_argument('--max-samples', type=int, default=None, help='score only the first N samples')
    p.add_argument('--out', default=None, help='directory of metrics.json (default: beside the samples)')
    p.add_argument('--swd', type=int, default=0, metavar='P', help='also report the exact sliced Wasserstein distance between the '
                   'patch distributions over P random directions with entries in {-1, 0, +1} (default 0: off)')
    p.add_argument('--swd-seed', type=int, default=0, help='seed of the directions')
    return p


def patch_score(d2, D):
    """coherence / completeness of one direction: mean_i d2[i] / (D * 255^2), from the integer sum (exactly 0.0 for a copy and
    exactly 1.0 for black against white)."""
    d2 = torch.as_tensor(d2)
    return int(d2.sum(dtype=torch.int64)) / (d2.numel() * int(D) * 255 * 255)


def nn_unique_frac(nn, Nr):
    """Distinct nearest-neighbour indices over min(Nq, Nr): low for a sample stitched from a few source patches."""
    nn = torch.as_tensor(nn)
    return int(torch.unique(nn).numel()) / min(int(nn.numel()), int(Nr))


def diversity(samples, real):
    """SinGAN's diversity: the mean over pixels of the standard deviation across samples of the channel-mean intensity, over the
    standard deviation of that intensity over the real volume (population standard deviations).  samples: uint8 [N,T,H,W,3] /
    [N,H,W,3], real: [T',H,W,3] / [H,W,3]; None when there are fewer than 2 samples, H or W differ, or the real volume is
    shorter than the samples (its first T frames are used)."""
    samples, real = torch.as_tensor(samples), torch.as_tensor(real)
    if samples.shape[0] < 2 or samples.dim() != real.dim() + 1:
        return None
    if samples.dim() == 5:
        T = samples.shape[1]
        if real.shape[0] < T:
            return None
        real = real[:T]
    if tuple(samples.shape[1:]) != tuple(real.shape):
        return None
    s = samples.to(torch.float64).mean(-1)
    r = real.to(torch.float64).mean(-1)
    denom = float(r.std(unbiased=False))
    if denom == 0.0:
        return None
    return float(s.std(0, unbiased=False).mean()) / denom


def swd_directions(P, D, seed):
    """int8 [P][D] directions for the sliced Wasserstein distance: entries drawn uniformly from {-1, 0, +1} by
    numpy.random.default_rng(seed) on the host, all-zero rows drawn again."""
    rng = np.random.default_rng(seed)
    dirs = rng.integers(-1, 2, size=(int(P), int(D)), dtype=np.int8)
    while True:
        zero = np.flatnonzero(~dirs.any(1))
        if len(zero) == 0:
            return dirs
        dirs[zero] = rng.integers(-1, 2, size=(len(zero), int(D)), dtype=np.int8)


def swd_score(num, Na, Nb, dirs):
    """Sliced Wasserstein distance from the integer numerators of ops.hist_w1: the mean over directions of
    num[p] / (Na * Nb * 255 * sqrt(nnz_p)), i.e. W1 along the unit vector dirs[p] / sqrt(nnz_p) in units of the full intensity
    range.  Exactly 0.0 when every numerator is 0 (equal patch multisets)."""
    num = [int(v) for v in (num.tolist() if hasattr(num, "tolist") else num)]
    nnz = [int(v) for v in np.count_nonzero(np.asarray(dirs), axis=1)]
    if len(num) != len(nnz) or not num:
        raise ValueError("swd_score: %d numerators for %d directions" % (len(num), len(nnz)))
    scale = int(Na) * int(Nb) * 255
    return sum((n / scale) / math.sqrt(z) for n, z in zip(num, nnz)) / len(num)   # n / scale: Python's correctly rounded int / int


def real_volume(opt, real_path=None, device=None):
    """The real volume the last stage was trained on, as uint8 [T,H,W,3] (images [H,W,3]) on the device: the run's input (or
    real_path) trimmed by start_frame / max_frames as the dataset does, frames 0, e, 2e, ... with e the last stage's sampling
    rate, resized to the last stage's size by the dataset's kernel (quantize on, no flip) and mapped back to its uint8 levels."""
    path = real_path or (opt.video_path if opt.dims == 3 else opt.image_path)
    frames = datasets.load_frames(path)
    size = datasets._stage_size(opt, opt.stop_scale)
    if opt.dims == 3:
        start = getattr(opt, "start_frame", 0)
        frames = frames[start:start + opt.max_frames] if getattr(opt, "max_frames", None) else frames[start:]
        every = opt.sampling_rates[hp_utils.get_fps_td_by_index(opt.stop_scale, opt)[2]]
        store = datasets._DeviceFrames(frames, device)
        return store.clip_u8(0, every, len(range(0, store.N, every)), size[0], size[1])
    store = datasets._DeviceFrames(frames[:1], device)
    return store.clip_u8(0, 1, 1, size[0], size[1])[0]


def evaluate(exp_dir=None, samples=None, real=None, patch=None, stride=(1, 1, 1), max_samples=None, out=None, swd=0, swd_seed=0):
    """Score `samples` against the real volume; writes metrics.json (and, with exp_dir, the real volume used as real.npy) into
    `out` and returns the metrics.  swd > 0: also the sliced Wasserstein patch distance over that many directions."""
    import types
    if exp_dir is None and (samples is None or real is None):
        raise SystemExit("evaluate: give --exp-dir, or both --samples and --real")
    spath = samples or os.path.join(exp_dir, 'eval', 'samples', 'samples.npy')
    if not os.path.isfile(spath):
        raise SystemExit("evaluate: no samples at {}; run `python -m hp_vae_gan_amd.generate --exp-dir {}` first "
                         "(or pass --samples)".format(spath, exp_dir or '<experiment>'))
    if not torch.cuda.is_available():
        raise SystemExit("hp-vae-gan_amd: no GPU visible; every op runs on an MI355X")
    device = torch.device('cuda', torch.cuda.current_device())
    arr = np.load(spath, allow_pickle=False)
    if arr.dtype != np.uint8 or arr.ndim not in (4, 5) or arr.shape[-1] != 3:
        raise SystemExit("evaluate: samples must be uint8 [N,T,H,W,3] or [N,H,W,3], got {} {}".format(arr.dtype, arr.shape))
    if max_samples:
        arr = arr[:max_samples]
    video = arr.ndim == 5
    out = out or os.path.dirname(os.path.abspath(spath))
    os.makedirs(out, exist_ok=True)
    if exp_dir is not None:
        with open(os.path.join(exp_dir, 'opt.json')) as f:
            opt = types.SimpleNamespace(**json.load(f))
        if (opt.dims == 3) != video:
            raise SystemExit("evaluate: the samples' rank does not match the experiment ({}-D)".format(opt.dims))
        real_dev = real_volume(opt, real, device)
        np.save(os.path.join(out, 'real.npy'), real_dev.cpu().numpy())
    else:
        ra = datasets.load_frames(real)
        if ra.dtype != np.uint8 or ra.shape[-1] != 3:
            raise SystemExit("evaluate: --real must be uint8 [...,3], got {} {}".format(ra.dtype, ra.shape))
        if not video and ra.ndim == 4:
            ra = ra[0]
        if ra.ndim != arr.ndim - 1:
            raise SystemExit("evaluate: --real {} does not match samples {}".format(ra.shape, arr.shape))
        real_dev = torch.from_numpy(np.ascontiguousarray(ra)).to(device)
    patch = tuple(patch) if patch else ((3, 7, 7) if video else (1, 7, 7))
    stride = tuple(stride)
    samples_dev = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
    vol = (lambda t: tuple(t.shape[:3])) if video else (lambda t: (1,) + tuple(t.shape[:2]))
    coh_counts = ops.patch_nn_counts(vol(samples_dev[0]), vol(real_dev), patch, qstride=stride)
    com_counts = ops.patch_nn_counts(vol(real_dev), vol(samples_dev[0]), patch, qstride=stride)
    D = coh_counts[2]
    per_sample = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    seconds = 0.0
    for smp in samples_dev:
        e0.record()
        d2c, nnc = ops.patch_nn(smp, real_dev, patch, qstride=stride)
        d2r, _ = ops.patch_nn(real_dev, smp, patch, qstride=stride)
        e1.record()
        e1.synchronize()
        seconds += e0.elapsed_time(e1) / 1e3
        per_sample.append({"coherence": patch_score(d2c, D), "completeness": patch_score(d2r, D),
                           "nn_unique_frac": nn_unique_frac(nnc, coh_counts[1])})
    n = len(per_sample)
    metrics = {"samples": os.path.abspath(spath), "num_samples": n, "patch": list(patch), "stride": list(stride),
               "Nq": coh_counts[0], "Nr": coh_counts[1], "D": D, "Nq_completeness": com_counts[0], "Nr_completeness": com_counts[1],
               "per_sample": per_sample, "patchnn_seconds": seconds, "diversity": diversity(samples_dev, real_dev)}
    for k in ("coherence", "completeness", "nn_unique_frac"):
        metrics[k] = sum(p[k] for p in per_sample) / n
    swd_text = ""
    if swd and swd > 0:
        # the sample side carries the stride, the real side stays dense (as for coherence); its histograms are made once
        dirs = swd_directions(swd, D, swd_seed)
        dirs_dev = torch.from_numpy(dirs).to(device)
        Ns, Nr = coh_counts[0], coh_counts[1]
        e0.record()
        hist_real = ops.patch_proj_hist(real_dev, patch, dirs_dev)
        nums = [ops.hist_w1(ops.patch_proj_hist(smp, patch, dirs_dev, stride), Ns, hist_real, Nr) for smp in samples_dev]
        e1.record()
        e1.synchronize()
        for p, num in zip(per_sample, nums):
            p["swd"] = swd_score(num.cpu(), Ns, Nr, dirs)
        metrics.update({"swd": sum(p["swd"] for p in per_sample) / n, "swd_directions": int(swd), "swd_seed": int(swd_seed),
                        "swd_seconds": e0.elapsed_time(e1) / 1e3})
        swd_text = " swd {:.6f}".format(metrics["swd"])
    with open(os.path.join(out, 'metrics.json'), 'w') as f:
        json.dump(metrics, f, indent=1, sort_keys=True)
    print("evaluate: {} samples, patch {} stride {}: coherence {:.6f} completeness {:.6f} nn_unique_frac {:.4f} diversity {}{} "
          "({:.3f} s in patch_nn) -> {}".format(n, list(patch), list(stride), metrics["coherence"], metrics["completeness"],
                                               metrics["nn_unique_frac"],
                                               "n/a" if metrics["diversity"] is None else "{:.4f}".format(metrics["diversity"]),
                                               swd_text, seconds, os.path.join(out, 'metrics.json')))
    return metrics


def evaluate_main(argv=None):
    a = evaluate_parser().parse_args(argv)
    evaluate(a.exp_dir, a.samples, a.real, a.patch, a.stride, a.max_samples, a.out, a.swd, a.swd_seed)
    return 0


# ------------------------------------------------------------------------------------------------------ generate_patchnn
# The training-free counterpart of the trained generator: GPNN (Granot et al., "Drop the GAN", CVPR 2022) and its video form
# VGPNN (Haim et al., ECCV 2022) on the exact patch engine of `evaluate`.  Everything is a uint8 volume [T,H,W,3]; an image is
# the volume with T = 1.  Coarse to fine over a spatial pyramid of the real volume (T is kept; a spatio-temporal pyramid is
# not built), every level repeats one step: search, for each patch of the current guess, the key patch that minimises
# d2 / (alpha_abs + the key's distance to ITS nearest guess patch) (the completeness normalisation: key patches the guess
# does not use yet become cheap), then vote the value patches of the winners into the next guess.
def generate_patchnn_parser():
    def alpha(s):
        v = float(s)
        if not v > 0:
            raise argparse.ArgumentTypeError("--alpha must be > 0 (inf: no completeness normalisation)")
        return v
    p = argparse.ArgumentParser(prog="python -m hp_vae_gan_amd.generate_patchnn",
                                description="Training-free samples of one clip / image by coarse-to-fine patch nearest "
                                "neighbours (GPNN / VGPNN) on the exact patch engine of `evaluate`.")
    p.add_argument('--exp-dir', default=None, help='experiment_<n> directory: the real volume is the one `evaluate` compares against')
    p.add_argument('--video-path', default=None, help='a clip taken as it is (.npy [N,H,W,3] uint8 or a frame directory); needs --out')
    p.add_argument('--image-path', default=None, help='an image taken as it is (.npy [H,W,3] uint8 or an image file); needs --out')
    p.add_argument('--out', default=None, help='output directory (default: <exp-dir>/eval/samples_patchnn)')
    p.add_argument('--num-samples', type=int, default=8, help='number of samples')
    p.add_argument('--seed', type=int, default=0, help='sample i draws its noise under seed + i')
    p.add_argument('--patch', type=int, nargs=3, default=None, metavar=('T', 'H', 'W'), help='patch (default 3 7 7, images 1 7 7)')
    p.add_argument('--ratio', type=float, default=0.75, help='size ratio between two levels of the pyramid')
    p.add_argument('--min-size', type=int, default=16, help='the coarsest level keeps min(H, W) >= this')
    p.add_argument('--iters', type=int, default=10, help='refine steps per level')
    p.add_argument('--alpha', type=alpha, default=0.005, help='completeness normalisation, in units of D * 255^2 (the unit of '
                   '`evaluate`\'s coherence); inf turns it off')
    p.add_argument('--noise', type=float, default=0.75, help='standard deviation, in units of 255, of the noise added to the coarsest guess')
    p.add_argument('--size', type=int, nargs=3, default=None, metavar=('T', 'H', 'W'), help='size of the samples (default: the real '
                   'volume\'s; another size retargets)')
    p.add_argument('--save-levels', action='store_true', help='also write levels.npz: the real pyramid (level_<l>) and the blurred '
                   'keys of every level above the coarsest (keys_<l>)')
    return p


def patchnn_pyramid_sizes(shape, ratio, min_size, patch=(3, 7, 7)):
    """[(T, H, W)] of the pyramid of a (T, H, W) volume from coarse to fine: level l of L has (H, W) scaled by ratio^(L-1-l) and
    rounded (halves up), the finest is the volume itself and T is kept.  L is the largest count whose coarsest level has
    min(H, W) >= min_size (at least 1).  Refuses a coarsest level smaller than the patch.  Host only."""
    T, H, W = (int(e) for e in shape)
    ratio = float(ratio)
    if not 0.0 < ratio < 1.0:
        raise ValueError("patchnn_pyramid_sizes: ratio must lie in (0, 1), got %r" % (ratio,))
    if min(T, H, W) < 1:
        raise ValueError("patchnn_pyramid_sizes: bad volume %s" % ((T, H, W),))

    def at(k):
        return T, int(math.floor(H * ratio ** k + 0.5)), int(math.floor(W * ratio ** k + 0.5))
    L = 1
    while min(at(L)[1:]) >= max(int(min_size), 1):
        L += 1
    sizes = [at(L - 1 - l) for l in range(L)]
    if any(s < p for s, p in zip(sizes[0], patch)):
        raise ValueError("patchnn_pyramid_sizes: the coarsest level %s is smaller than the patch %s (raise min_size)"
                         % (sizes[0], tuple(patch)))
    return sizes


def _resize_u8(vol, size):
    """uint8 [T,H,W,3] -> uint8 [*size, 3]: the trilinear align-corners resize (ops.UpsampleAC, fp32), rounded and clamped."""
    size = tuple(int(e) for e in size)
    if tuple(vol.shape[:3]) == size:
        return vol.contiguous()
    x = vol.permute(3, 0, 1, 2)[None].to(torch.float32).contiguous()
    with torch.no_grad():
        y = ops.UpsampleAC.apply(x, size, None, 0.0)
    return torch.round(y).clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 3, 0).contiguous()


def patchnn_real_levels(real, sizes):
    """(levels, keys) of the real volume [T,H,W,3]: levels[l] is the full-size volume resized to sizes[l]; keys[l] (l > 0) is
    levels[l-1] resized to sizes[l], the blurred keys of the first step of level l (keys[0] is levels[0])."""
    levels = [_resize_u8(real, s) for s in sizes]
    keys = [levels[0]] + [_resize_u8(levels[l - 1], sizes[l]) for l in range(1, len(sizes))]
    return levels, keys


def patchnn_weights(m, alpha_abs):
    """w = 1 / (float32(m) + float32(alpha_abs)) for the int32 distances m: one fp32 add and one correctly rounded fp32 divide
    per key patch (the generator's results are defined bit for bit, so this must equal numpy's float32 arithmetic)."""
    return 1.0 / (m.to(torch.float32) + torch.tensor(alpha_abs, dtype=torch.float32, device=m.device))


def patchnn_refine(query, keys, values, patch, alpha_abs, return_score=False):
    """One GPNN step on uint8 volumes (or images): m = for every key patch the distance to its nearest query patch,
    w = 1 / (float32(m) + float32(alpha_abs)), nn = the weighted nearest key of every query patch, result = the vote of the
    value patches nn (keys and values share one grid) with the query as fallback.  alpha_abs = inf: the plain nearest key,
    one search.  return_score: also the mean of the minimised quantity (d2 * w; d2 for inf)."""
    if math.isinf(alpha_abs):
        score, nn = ops.patch_nn(query, keys, patch)
    else:
        m, _ = ops.patch_nn(keys, query, patch)
        score, nn = ops.patch_nn_weighted(query, keys, patchnn_weights(m, alpha_abs), patch)
    out = ops.patch_vote(values, nn, patch, tuple(query.shape[:-1]), query)
    if return_score:
        return out, float(score.to(torch.float64).mean())
    return out


def patchnn_synthesize(real, size=None, patch=None, ratio=0.75, min_size=16, iters=10, noise=0.75, alpha=0.005, seed=0, index=0,
                       pyramid=None):
    """One sample of the uint8 device volume `real` ([T,H,W,3]; images [H,W,3]) -> (sample, mean final score).  size: the
    sample's (T, H, W) (default real's).  The coarsest guess is real level 0 (resized to the sample's coarsest size) plus
    noise * 255 * N(0, 1) drawn under torch.manual_seed(seed + index); level 0 runs `iters` steps with keys = values = real
    level 0; level l > 0 starts from the previous result resized, runs one step with the blurred keys (real level l-1 resized
    to level l) and values real level l, then iters - 1 steps with keys = values = real level l.  pyramid: a
    (sizes, levels, keys) triple of patchnn_pyramid_sizes / patchnn_real_levels to reuse between samples."""
    image = real.dim() == 3
    vol = real[None] if image else real
    patch = tuple(patch) if patch else ((1, 7, 7) if image else (3, 7, 7))
    if pyramid is None:
        sizes = patchnn_pyramid_sizes(vol.shape[:3], ratio, min_size, patch)
        pyramid = (sizes,) + patchnn_real_levels(vol, sizes)
    sizes, levels, keys = pyramid
    L = len(sizes)
    if size is None or tuple(size) == tuple(vol.shape[:3]):
        qsizes = sizes
    else:
        St, Sh, Sw = (int(e) for e in size)
        qsizes = [(St, int(math.floor(Sh * ratio ** (L - 1 - l) + 0.5)), int(math.floor(Sw * ratio ** (L - 1 - l) + 0.5)))
                  for l in range(L)]
        if any(s < p for s, p in zip(qsizes[0], patch)):
            raise ValueError("patchnn_synthesize: the sample's coarsest level %s is smaller than the patch %s" % (qsizes[0], patch))
    alpha_abs = float(alpha) * 3 * patch[0] * patch[1] * patch[2] * 255 * 255
    iters = max(int(iters), 1)
    q = _resize_u8(levels[0], qsizes[0])
    if noise:
        torch.manual_seed(int(seed) + int(index))
        with ops.noise_stream(q.device):
            z = ops.normal_(torch.empty(q.shape, dtype=torch.float32, device=q.device))
        q = torch.round(q.to(torch.float32) + (float(noise) * 255.0) * z).clamp_(0, 255).to(torch.uint8)
    score = None
    for l in range(L):
        if l > 0:
            q = _resize_u8(q, qsizes[l])
        for it in range(iters):
            k = keys[l] if (l > 0 and it == 0) else levels[l]
            q, score = patchnn_refine(q, k, levels[l], patch, alpha_abs, return_score=True)
    return (q[0] if image else q), score


def generate_patchnn(exp_dir=None, video_path=None, image_path=None, out=None, num_samples=8, seed=0, patch=None, ratio=0.75,
                     min_size=16, iters=10, alpha=0.005, noise=0.75, size=None, save_levels=False):
    """Write samples.npy (uint8 [N,T,H,W,3], images [N,H,W,3]: what `evaluate --samples` reads), one GIF / PNG per sample and
    patchnn.json (the settings, the level sizes, seconds per sample from HIP events, the mean final score per sample)."""
    import types
    given = [a for a in (exp_dir, video_path, image_path) if a is not None]
    if len(given) != 1:
        raise SystemExit("generate_patchnn: give exactly one of --exp-dir, --video-path and --image-path")
    if exp_dir is None and out is None:
        raise SystemExit("generate_patchnn: --video-path / --image-path need --out")
    if not torch.cuda.is_available():
        raise SystemExit("hp-vae-gan_amd: no GPU visible; every op runs on an MI355X")
    device = torch.device('cuda', torch.cuda.current_device())
    fps = 10
    if exp_dir is not None:
        with open(os.path.join(exp_dir, 'opt.json')) as f:
            opt = types.SimpleNamespace(**json.load(f))
        real = real_volume(opt, None, device)
        if opt.dims == 3:
            fps = hp_utils.get_fps_td_by_index(opt.stop_scale, opt)[0]
        out = out or os.path.join(exp_dir, 'eval', 'samples_patchnn')
    else:
        ra = datasets.load_frames(video_path or image_path)
        if ra.dtype != np.uint8 or ra.ndim not in (3, 4) or ra.shape[-1] != 3:
            raise SystemExit("generate_patchnn: the input must be uint8 [N,H,W,3] or [H,W,3], got {} {}".format(ra.dtype, ra.shape))
        if image_path is not None and ra.ndim == 4:
            ra = ra[0]
        if video_path is not None and ra.ndim == 3:
            ra = ra[None]
        real = torch.from_numpy(np.ascontiguousarray(ra)).to(device)
    image = real.dim() == 3
    vol = real[None] if image else real
    patch = tuple(patch) if patch else ((1, 7, 7) if image else (3, 7, 7))
    size = tuple(size) if size else tuple(vol.shape[:3])
    try:
        sizes = patchnn_pyramid_sizes(vol.shape[:3], ratio, min_size, patch)
    except ValueError as e:
        raise SystemExit("generate_patchnn: {}".format(e))
    if image and size[0] != 1:
        raise SystemExit("generate_patchnn: an image's --size has T = 1")
    pyramid = (sizes,) + patchnn_real_levels(vol, sizes)
    os.makedirs(out, exist_ok=True)
    if save_levels:
        np.savez(os.path.join(out, 'levels.npz'), **{"level_%d" % l: v.cpu().numpy() for l, v in enumerate(pyramid[1])},
                 **{"keys_%d" % l: v.cpu().numpy() for l, v in enumerate(pyramid[2]) if l > 0})
    samples, seconds, scores = [], [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(num_samples):
        e0.record()
        try:
            smp, score = patchnn_synthesize(vol, size, patch, ratio, min_size, iters, noise, alpha, seed, i, pyramid)
        except ValueError as e:
            raise SystemExit("generate_patchnn: {}".format(e))
        e1.record()
        e1.synchronize()
        seconds.append(e0.elapsed_time(e1) / 1e3)
        scores.append(score)
        samples.append((smp[0] if image else smp).cpu().numpy())
    arr = np.stack(samples)
    np.save(os.path.join(out, 'samples.npy'), arr)
    ext = '.png' if image else '.gif'
    for i, a in enumerate(arr):
        write_frames(a, os.path.join(out, 'sample_{:04d}{}'.format(i, ext)), fps)
    info = {"input": os.path.abspath(exp_dir or video_path or image_path), "real_shape": list(vol.shape[:3]), "size": list(size),
            "num_samples": int(num_samples), "seed": int(seed), "patch": list(patch), "ratio": float(ratio), "min_size": int(min_size),
            "iters": int(iters), "alpha": (float(alpha) if math.isfinite(alpha) else "inf"), "noise": float(noise),
            "level_sizes": [list(s) for s in sizes], "seconds_per_sample": seconds, "final_score_per_sample": scores,
            "final_score": "mean over the sample's patches of the last step's minimum: d2 / (alpha D 255^2 + the key's distance "
                           "to its nearest sample patch); plain d2 for alpha = inf"}
    with open(os.path.join(out, 'patchnn.json'), 'w') as f:
        json.dump(info, f, indent=1, sort_keys=True)
    print("wrote {} patch nearest-neighbour samples {} ({} levels, {:.3f} s per sample) to {}".format(
        len(arr), tuple(arr.shape[1:]), len(sizes), sum(seconds) / max(len(seconds), 1), out))
    return arr


def generate_patchnn_main(argv=None):
    a = generate_patchnn_parser().parse_args(argv)
    generate_patchnn(a.exp_dir, a.video_path, a.image_path, a.out, a.num_samples, a.seed, a.patch, a.ratio, a.min_size, a.iters,
                     a.alpha, a.noise, a.size, a.save_levels)
    return 0


def main_guard(fn):
    sys.exit(fn())
