"""What more than one program uses, and the HP-VAE-GAN trainer behind `python -m hp_vae_gan_amd.train_video` and
`.train_image`.  Each program is its own module (train_video, train_image, train_video_baselines, generate, evaluate,
generate_patchnn); those import from here and never from each other, since a module run with -m is loaded as __main__ and
a second import under its own name would load it twice.

Shared: the flags every trainer holds (trainer_parser), the run directory, the logbook, frames on disk, the trainer setup and
stage loop (Program, which train_video_baselines.BaselineProgram adjusts), and the helpers of the sampling and scoring
programs: gpu_device, load_opt, default_patch, load_u8_frames, write_samples, real_volume, the hole-mask readers (mask_forms,
pick_mask) and the --guide flags of generate and generate_patchnn (add_guide_flags, check_guide_flags, load_guide_frames).

The trainers follow the reference's programs (train_video.py:265-417, train_image.py:279-440): the same flags, the same
setup (noise_amp_init / scale_factor_init, adjust_scales2image, manualSeed drawn when absent and logged, then random.seed
and torch.manual_seed), a shuffled DataLoader that drops the last short batch over a dataset that serves device tensors (so
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

Snapshots (snapshot.py; this project's own): --snapshot-interval K writes <experiment>/snapshot.pth after every K-th iteration
of a stage (3 <= k < niter, after the iteration's preview and drain) and after every stage's checkpoints; --snapshot-exit-after
N ends the process cleanly after the N-th; --resume EXP_DIR continues that run in its directory.  The three flags are added on
top of build_parser's (Program.parser) and settled before the device is asked for (snapshot.resolve); they are no settings of
the experiment and stay out of opt.json.  A resume runs this same setup from the command line the snapshot recorded (seed
included), appends to scalars.jsonl (cut back to the recorded length) and logbook.txt, leaves opt.json alone, grows the
generator to the snapshot's stage and either goes on with the next stage (a finished one) or builds the stage the normal way
and puts the state into it (train.train's `resume`).  Stopped and resumed any number of times the run leaves the checkpoints
and scalars.jsonl of the run that was never stopped, bit for bit; with the flags absent nothing here does anything new.

Not built: mp4 decoding / encoding (cv2), tensorboard event files and neptune (--tag is only recorded), a CPU path
(--no-cuda is refused), multi-GPU launch."""
import argparse
import glob
import json
import os
import random
import sys
import types

import numpy as np
import torch

from . import checkpoint, datasets, ops, snapshot, telemetry
from . import train as hp_train
from . import utils as hp_utils
from .modules import networks_2d, networks_3d

# column of the loss log -> the reference's scalar tag (train_video.py:210-222) or a tag of its own
TAGS = {"rec_vae_loss": "Rec VAE", "kl_loss": "KLD", "rec_loss": "rec loss", "errG": "errG", "errD_real": "errD_real",
        "errD_fake": "errD_fake", "gradient_penalty": "gradient_penalty", "total_loss": "total_loss", "grad_norm": "grad_norm"}


# ------------------------------------------------------------------------------------------------------------------- flags
def trainer_parser(name, description, video=True):
    """A parser `python -m hp_vae_gan_amd.<name>` with the flags every trainer holds: those the reference's train_video.py,
    train_image.py (video=False) and train_video_baselines.py share, with their names, types, defaults and `required`, plus
    --run-dir and --no-hip-graph.  The caller adds what is its own; --generator, --discriminator, --mode and --visualize are
    among that, since their defaults or help differ from trainer to trainer."""
    p = argparse.ArgumentParser(prog="python -m hp_vae_gan_amd." + name, description=description)
    a = p.add_argument
    # load, input, save
    a('--netG', default='', help='netG.pth of an experiment to resume from (its scale is trained again)')
    a('--netD', default='', help='accepted, unused (as in the reference)')
    a('--manualSeed', type=int, help='seed of python random and torch (random when absent)')
    # networks
    a('--nc-im', type=int, default=3, help='image channels')
    a('--nfc', type=int, default=64, help='base channel count')
    a('--ker-size', type=int, default=3, help='kernel size')
    a('--num-layer', type=int, default=5, help='layers per block')
    a('--stride', default=1, help='stride')
    a('--padd-size', type=int, default=1, help='padding')
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
    a('--disc-loss-weight', type=float, default=1.0, help='adversarial loss weight')
    a('--lr-scale', type=float, default=0.2, help='learning-rate scaling of the lower trained levels')
    a('--train-depth', type=int, default=1, help='levels trained at once')
    # data
    if video:
        a('--video-path', required=True, help='frame directory or .npy [N,H,W,3] uint8 (no mp4 decoder in this build)')
        a('--start-frame', default=0, type=int, help='first frame')
        a('--max-frames', default=1000, type=int, help='frames to keep')
        a('--sampling-rates', type=int, nargs='+', default=[4, 3, 2, 1], help='temporal sampling rates')
    a('--hflip', action='store_true', default=False, help='random horizontal flips')
    a('--img-size', type=int, default=256)
    a('--stop-scale-time', type=int, default=-1)
    a('--data-rep', type=int, default=1 if video else 1000, help='dataset repetitions')
    # main
    a('--checkname', type=str, default='DEBUG', help='run name')
    a('--batch-size', type=int, default=2, help='batch size')
    a('--print-interval', type=int, default=100, help='iterations between log drains (and previews)')
    a('--no-cuda', action='store_true', default=False, help='refused: there is no CPU path')
    # this project's own
    a('--run-dir', default='run', help='root of the run directories')
    a('--no-hip-graph', action='store_true', default=False, help='stay eager (no hipGraph replay)')
    p.set_defaults(hflip=False)
    return p


def check_tap_flags(ker_size, padd_size):
    """End the program on a --ker-size the convolutions do not have, or a --padd-size that does not keep the generator's levels
    'same' for a --ker-size of 5 or 7 (--ker-size 1 and 3 are taken as before)."""
    if ker_size in (1, 3):
        return
    if ker_size not in (5, 7):
        raise SystemExit("--ker-size {}: the convolutions run 3, 5 or 7 taps per axis (and 1)".format(ker_size))
    if padd_size != ker_size // 2:
        raise SystemExit("--ker-size {} needs --padd-size ker_size // 2 = {} (got {}): every generator level adds its block's "
                         "output to its input, so the block must keep the size".format(ker_size, ker_size // 2, padd_size))


def build_parser(kind):
    """The reference's parser of train_video.py (kind 'video') or train_image.py ('image'): same names, types, defaults and
    `required`; plus --run-dir and --no-hip-graph."""
    video = kind == "video"
    p = trainer_parser("train_" + kind, "Train HP-VAE-GAN on one %s, stage by stage, on an MI355X." % kind, video)
    a = p.add_argument
    a('--latent-dim', type=int, default=128, help='VAE latent channels')
    a('--vae-levels', type=int, default=3, help='number of VAE levels')
    a('--enc-blocks', type=int, default=2, help='encoder blocks')
    a('--generator', type=str, default='GeneratorHPVAEGAN', help='generator class')
    a('--discriminator', type=str, default='WDiscriminator3D' if video else 'WDiscriminator2D', help='discriminator class')
    a('--rec-weight', type=float, default=10., help='reconstruction loss weight')
    a('--kl-weight', type=float, default=1., help='KL weight')
    a('--grad-clip', type=float, default=5, help='gradient clip norm')
    a('--const-amp', action='store_true', default=False, help='constant noise amplitude')
    a('--train-all', action='store_true', default=False, help='train all levels w.r.t. train-depth')
    a('--mode', default='train', help='task')
    a('--visualize', action='store_true', default=False, help='write previews (GIF / PNG) under previews/')
    if not video:
        a('--image-path', required=True, help='image file, directory of images or .npy [N,H,W,3] uint8')
        a('--tag', type=str, default='', help='recorded in opt.json only (the reference tags a neptune run)')
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


def load_opt(exp_dir):
    """The settings of an experiment directory (its opt.json) as a namespace."""
    with open(os.path.join(exp_dir, 'opt.json')) as f:
        return types.SimpleNamespace(**json.load(f))


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


# ------------------------------------------------------------------------------------------------- device, frames, samples
def gpu_device():
    """The current GPU; no GPU ends the program."""
    if not torch.cuda.is_available():
        raise SystemExit("hp-vae-gan_amd: no GPU visible; every op runs on an MI355X")
    return torch.device('cuda', torch.cuda.current_device())


def default_patch(video):
    """The patch of `evaluate` and `generate_patchnn` when none is given: (T, H, W) = 3 7 7, images 1 7 7."""
    return (3, 7, 7) if video else (1, 7, 7)


def load_u8_frames(path, device, image, complaint, ranks=None):
    """Raw frames taken as they are (.npy, frame directory or image file) as a uint8 device tensor [...,3]; an image keeps
    only the first of several frames.  Another dtype, a rank outside `ranks` when those are given, or another channel count ends
    the program with `complaint` (the caller's name and what it wants) and the dtype and shape found."""
    ra = datasets.load_frames(path)
    if ra.dtype != np.uint8 or (ranks and ra.ndim not in ranks) or ra.shape[-1] != 3:
        raise SystemExit("{}, got {} {}".format(complaint, ra.dtype, ra.shape))
    if image and ra.ndim == 4:
        ra = ra[0]
    return torch.from_numpy(np.ascontiguousarray(ra)).to(device)


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


def write_samples(out, arr, fps):
    """Write the uint8 samples [N,T,H,W,3] (images [N,H,W,3]) into the directory `out`: samples.npy, which `evaluate --samples`
    reads, and one GIF (PNG) per sample."""
    os.makedirs(out, exist_ok=True)
    np.save(os.path.join(out, 'samples.npy'), arr)
    ext = '.gif' if arr.ndim == 5 else '.png'
    for i, a in enumerate(arr):
        write_frames(a, os.path.join(out, 'sample_{:04d}{}'.format(i, ext)), fps)


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


# ------------------------------------------------------------------------------------------------------------ training
def networks_of(opt):
    return networks_3d if opt.dims == 3 else networks_2d


def _stage_data(loader, holder, pos=None):
    """Iterate the DataLoader and remember the batch at hand (the previews show `real`).  pos: the snapshot.LoaderPosition of
    a run with snapshots (it counts the batches and remembers the epoch's start), else None."""
    return snapshot.iterate(loader, pos, holder)


class _Loop:
    """Re-iterable view of the DataLoader that remembers the batch at hand (train.train restarts an exhausted iterator)."""

    def __init__(self, loader, holder, pos=None):
        self.loader, self.holder, self.pos = loader, holder, pos

    def __iter__(self):
        return _stage_data(self.loader, self.holder, self.pos)


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
        # after the preview and the drain: the BatchNorm buffers a preview moved are in the file
        k = trainer.iteration
        if self.prog.snap_interval and k % self.prog.snap_interval == 0 and 3 <= k < opt.niter:
            self.prog.write_snapshot(trainer, self.log, False)


class Program:
    """One training run of train_video / train_image (see the module docstring).  train_video_baselines.BaselineProgram is
    this run with the baselines' parser, critic, loss-log columns, train function and Z_init: the members up to end_stage are
    what it replaces."""

    tags = TAGS                                  # loss-log column -> scalar tag
    program = None                               # opt.json's "program" (`generate` tells the baselines' runs by it)
    train_fn = staticmethod(hp_train.train)      # trains one stage

    def parser(self):
        return snapshot.add_flags(build_parser(self.kind))

    def program_name(self):
        return self.program or 'train_' + self.kind

    def check_taps(self, opt):
        """--ker-size / --padd-size, before anything is set up: 5 and 7 taps run with the padding that keeps the generator's
        levels 'same' (the residual of every level adds the block's output to its input)."""
        check_tap_flags(opt.ker_size, opt.padd_size)

    def check_flags(self, opt):
        assert opt.vae_levels > 0
        if self.kind == 'image' and opt.data_rep < opt.batch_size:
            opt.data_rep = opt.batch_size

    def logs_noise_amp(self):
        return True

    def begin_stage(self):
        """Before the stage's discriminator is made."""

    def make_discriminator(self):
        opt = self.opt
        if not opt.vae_levels < opt.scale_idx + 1:
            return None
        netD = getattr(networks_of(opt), opt.discriminator)(opt).to(opt.device)
        if opt.netG != '' and opt.resumed_idx == opt.scale_idx:
            checkpoint.warm_start_discriminator(netD, opt.resume_dir, opt.scale_idx)
        elif opt.vae_levels < opt.scale_idx:
            checkpoint.warm_start_discriminator(netD, self.exp_dir, opt.scale_idx)
        return netD

    def loss_columns(self, netD):
        return hp_train.loss_log_columns(netD is not None)

    def end_stage(self, trainer):
        """After the stage's last drain, before its checkpoints."""

    # ---- setup
    def __init__(self, kind, argv=None):
        self.kind = kind
        # the snapshot flags are settled first and before the device is asked for: --resume brings the whole command line
        # of the run it continues, and --video-path / --image-path are `required`
        argv, flags, self.resume_snapshot = snapshot.resolve(sys.argv[1:] if argv is None else argv, self.program_name())
        opt = self.parser().parse_args(argv)
        self.check_taps(opt)
        for name in ('snapshot_interval', 'snapshot_exit_after', 'resume'):
            delattr(opt, name)   # the run's own business, not a setting of the experiment (opt.json stays what it was)
        self.snap_interval, self.snap_exit_after = flags.snapshot_interval, flags.snapshot_exit_after
        self.snapshots_written = 0
        self.loader_pos = None
        self.restore_skip, self.restore_verify = (), True   # test hooks of snapshot.restore
        seed_given = opt.manualSeed is not None
        if opt.no_cuda:
            raise SystemExit("--no-cuda: hp-vae-gan_amd has no CPU path; every op runs on an MI355X")
        self.path = opt.video_path if kind == 'video' else opt.image_path
        if self.path.lower().endswith('.mp4') or not os.path.exists(self.path):
            datasets.load_frames(self.path)   # the data front-end's own error (no decoder / missing file)
        opt.device = gpu_device()
        self.check_flags(opt)
        assert opt.disc_loss_weight > 0
        if self.program:
            opt.program = self.program
        opt.dims = 3 if kind == 'video' else 2
        opt.hip_graph = not opt.no_hip_graph
        if self.resume_snapshot is not None:
            self.exp_dir = os.path.normpath(flags.resume)
            snapshot.truncate_scalars(os.path.join(self.exp_dir, 'scalars.jsonl'), self.resume_snapshot['scalars_bytes'])
        else:
            self.exp_dir = experiment_dir(opt.run_dir, clip_name(self.path), opt.checkname)
        opt.experiment_dir = self.exp_dir
        self.log = Logbook(os.path.join(self.exp_dir, 'logbook.txt'))
        self.scalars = open(os.path.join(self.exp_dir, 'scalars.jsonl'), 'a')
        opt.noise_amp_init = opt.noise_amp
        opt.scale_factor_init = opt.scale_factor
        hp_utils.adjust_scales2image(opt.img_size, opt)
        if opt.manualSeed is None:
            opt.manualSeed = random.randint(1, 10000)
        self.log("Random Seed: {}".format(opt.manualSeed))
        self.recorded_argv = snapshot.recorded_command_line(argv, opt.manualSeed, seed_given)
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
        if self.resume_snapshot is None:
            with open(os.path.join(self.exp_dir, 'opt.json'), 'w') as f:
                json.dump(json_settings(opt), f, indent=1, sort_keys=True)
        for k, v in json_settings(opt).items():
            self.log('{}: {}'.format(k, v))
        self.log("Experiment: {}".format(self.exp_dir))
        self.netG = getattr(networks_of(opt), opt.generator)(opt).to(opt.device)
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
    def train_stage(self, resume=None):
        opt = self.opt
        if opt.dims == 3:
            opt.fps, opt.td, opt.fps_index = hp_utils.get_fps_td_by_index(opt.scale_idx, opt)
            self.log("Scale {}: FPS {}, time depth {}, sampling rate {}".format(
                opt.scale_idx, opt.fps, opt.td, opt.sampling_rates[opt.fps_index]))
            self.dataset.generate_frames(opt.scale_idx)
        self.begin_stage()
        netD = self.make_discriminator()
        log = telemetry.LossLog(self.loss_columns(netD), capacity=max(64, 2 * opt.print_interval), device=opt.device)
        holder = [None]
        self.loader_pos = snapshot.LoaderPosition() if self.snap_interval or resume is not None else None
        more = {}
        if resume is not None:   # a mid-stage snapshot: the stage is built the normal way, then the state goes into it
            def put_back(trainer):
                self.resumed_trainer = trainer
                snapshot.restore(self, trainer, log, resume, skip=self.restore_skip, verify=self.restore_verify)
            more['resume'] = put_back
        trainer = self.train_fn(opt, self.netG, _Loop(self.loader, holder, self.loader_pos), netD=netD, loss_log=log,
                                callback=_Stage(self, log, holder), **more)
        if trainer.iteration % opt.print_interval != 0:
            self.drain(log)
        self.end_stage(trainer)
        checkpoint.save_stage(self.exp_dir, opt, trainer)
        self.trainers.append(trainer)
        self.logs.append(log)
        if self.snap_interval:
            self.write_snapshot(trainer, log, True)
        return trainer

    def write_snapshot(self, trainer, log, stage_done):
        """Drain the loss log, then write <experiment>/snapshot.pth (snapshot.collect); the logbook line carries the state
        digest, so two runs can be compared along the way.  --snapshot-exit-after: snapshot.ExitAfter after the N-th."""
        opt = self.opt
        self.drain(log)
        snap = snapshot.collect(self, trainer, log, stage_done)
        size = snapshot.write(self.exp_dir, snap)
        self.snapshots_written += 1
        self.log("Snapshot: stage {}, iteration {}/{}{}, {} bytes, digest {:016x}".format(
            opt.scale_idx, trainer.iteration, opt.niter, ' (stage done)' if stage_done else '', size, snap['digest']))
        if self.snap_exit_after and self.snapshots_written == self.snap_exit_after:
            raise snapshot.ExitAfter(self.snapshots_written)

    def run(self):
        try:
            self.run_stages()
        except snapshot.ExitAfter:
            torch.cuda.synchronize()
            self.log("Stopped after snapshot {} of this process (--snapshot-exit-after): continue with --resume {}".format(
                self.snapshots_written, self.exp_dir))
            self.scalars.close()
            self.log.close()
        return self

    def run_stages(self):
        opt = self.opt
        plan = stage_plan(opt.scale_idx, opt.resumed_idx, opt.stop_scale)
        snap, pending = self.resume_snapshot, None
        if snap is not None:
            # the generator grows to the snapshot's stage; a finished stage is restored here and the loop goes on with the
            # next one as the uninterrupted run does, an unfinished one is built below and restored inside train_stage
            for _ in range(snap['stage'] - opt.scale_idx):
                self.netG.init_next_stage()
            self.netG.to(opt.device)
            opt.scale_idx = snap['stage']
            snapshot.restore_settings(self, snap)
            self.log("Resumed from {}: stage {}, iteration {}/{}{}, digest {:016x}".format(
                os.path.join(self.exp_dir, snapshot.FILE), snap['stage'], snap['iteration'], snap['niter'],
                ' (stage done)' if snap['stage_done'] else '', snap['digest']))
            if snap['stage_done']:
                snapshot.restore_finished_stage(self, snap, skip=self.restore_skip, verify=self.restore_verify)
                plan = [(s, s > snap['stage']) for s, _ in plan if s > snap['stage']]
            else:
                pending = snap
                plan = [(s, s > snap['stage']) for s, _ in plan if s >= snap['stage']]
        for scale, grow in plan:
            opt.scale_idx = scale
            if grow:
                self.netG.init_next_stage()
                self.netG.to(opt.device)
            self.train_stage(resume=pending)
            pending = None
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

    def preview_items(self, real, out):
        """[(name, tensor)] of one preview: this iteration's batch and outputs and the random draws of `sample`."""
        fake_var, fake_vae_var = self.sample()
        return [('real', real), ('generated', out['generated']), ('generated_vae', out['generated_vae']),
                ('fake_var', fake_var), ('fake_vae_var', fake_vae_var)]

    def preview(self, trainer, out, batch, iteration):
        opt = self.opt
        items = self.preview_items(batch[0] if isinstance(batch, (list, tuple)) else batch, out)
        d = os.path.join(self.exp_dir, 'previews')
        os.makedirs(d, exist_ok=True)
        ext = '.gif' if opt.dims == 3 else '.png'
        fps = getattr(opt, 'fps', 1)
        for name, x in items:
            u8 = ops.video_to_u8(x.float()).cpu().numpy()
            for b in range(u8.shape[0]):
                write_frames(u8[b], os.path.join(d, 'scale{}_iter{:06d}_{}_{}{}'.format(opt.scale_idx, iteration, name, b, ext)),
                             fps)


def train_main(kind, argv=None):
    Program(kind, argv).run()
    return 0


# Hole masks (generate_patchnn --mask, --guide-mask of generate and generate_patchnn): what the programs share.
def mask_forms(path, who="generate_patchnn: --mask"):
    """Every [T,H,W] bool reading of a mask input, as host arrays: a .npy [T,H,W] or [H,W] (bool or uint8) as it is, and an
    input with a last axis of 3 ([...,3] .npy, an image file, a frame directory) with any nonzero channel as hole.  An array
    [H,W,3] has both readings; the volume's shape decides between them (pick_mask).  Another dtype or rank ends the program,
    under the program and flag `who`."""
    ra = datasets.load_frames(path)
    if ra.dtype not in (np.bool_, np.uint8):
        raise SystemExit("{} must be bool or uint8, got {} {}".format(who, ra.dtype, ra.shape))
    forms = ([ra] if ra.ndim in (2, 3) else []) + ([ra.any(-1)] if ra.ndim in (3, 4) and ra.shape[-1] == 3 else [])
    if not forms:
        raise SystemExit("{} must be [T,H,W], [H,W] or either with a last axis of 3, got {}".format(who, ra.shape))
    return [np.ascontiguousarray((m[None] if m.ndim == 2 else m) != 0) for m in forms]


def pick_mask(forms, shape, who="generate_patchnn: --mask", what="the real volume's"):
    """The reading of mask_forms with the volume's (T, H, W) = shape; none ends the program."""
    for m in forms:
        if tuple(m.shape) == tuple(shape):
            return m
    raise SystemExit("{} must have {} shape {}, got {}".format(
        who, what, tuple(shape), " or ".join(str(tuple(m.shape)) for m in forms)))


def refuse_trivial_mask(forms, who="generate_patchnn: --mask"):
    """End the program when every reading in `forms` is empty, or every one is all hole."""
    if all(not m.any() for m in forms) or all(m.all() for m in forms):
        raise SystemExit("{} is {}".format(who, "empty" if not forms[0].any() else "all hole"))


# Guided sampling (generate --guide, generate_patchnn --guide): the flags, their refusals and the guide's frames.
GUIDE_FEATHER = (1, 5, 5)          # --guide-feather of a clip; an image has RT = 0
GUIDE_FEATHER_MAX = 64             # ops.mask_blend's largest radius


def add_guide_flags(p):
    """The four flags both sampling programs take, with defaults that leave a run without them as it was."""
    p.add_argument('--guide', default=None, metavar='PATH', help='start from this clip / image (.npy, a frame directory or an image '
                   'file) injected at pyramid level --guide-level, instead of from noise: the levels above re-render it with the '
                   'input\'s own statistics')
    p.add_argument('--guide-level', type=int, default=None, metavar='N', help='the pyramid level (0 = coarsest) that takes the guide; '
                   'required with --guide')
    p.add_argument('--guide-mask', default=None, metavar='PATH', help='keep the samples only inside this hole mask (the forms of '
                   'generate_patchnn --mask; nonzero = hole) and the guide elsewhere, feathered by --guide-feather')
    p.add_argument('--guide-feather', type=int, nargs=3, default=None, metavar=('RT', 'RH', 'RW'), help='dilation and feather radius '
                   'of --guide-mask per axis, each in [0, {}] (default {} {} {}; images 0 {} {}, RT must be 0)'.format(
                       GUIDE_FEATHER_MAX, *GUIDE_FEATHER, *GUIDE_FEATHER[1:]))
    return p


def check_guide_flags(who, guide, guide_level, guide_mask, guide_feather, image):
    """The refusals of the --guide flags that need no device and no other input, under the program name `who`.  Returns
    (feather, forms): the feather in force ((rt, rh, rw), None without --guide-mask) and the readings of the mask (mask_forms,
    None without one); (None, None) without --guide.  image: the run is an image run (the feather's default, and RT = 0)."""
    if guide is None:
        for flag, v in (('--guide-level', guide_level), ('--guide-mask', guide_mask), ('--guide-feather', guide_feather)):
            if v is not None:
                raise SystemExit("{}: {} needs --guide".format(who, flag))
        return None, None
    if guide_level is None:
        raise SystemExit("{}: --guide needs --guide-level (the pyramid level that takes the guide)".format(who))
    if guide_feather is not None:
        guide_feather = tuple(int(e) for e in guide_feather)
        if len(guide_feather) != 3 or min(guide_feather) < 0 or max(guide_feather) > GUIDE_FEATHER_MAX:
            raise SystemExit("{}: --guide-feather takes RT RH RW, each in [0, {}], got {}".format(
                who, GUIDE_FEATHER_MAX, list(guide_feather)))
        if guide_mask is None:
            raise SystemExit("{}: --guide-feather needs --guide-mask".format(who))
        if image and guide_feather[0] != 0:
            raise SystemExit("{}: --guide-feather of an image has RT = 0, got {}".format(who, list(guide_feather)))
    if guide_mask is None:
        return None, None
    feather = guide_feather if guide_feather is not None else ((0,) + GUIDE_FEATHER[1:] if image else GUIDE_FEATHER)
    forms = mask_forms(guide_mask, who + ": --guide-mask")
    refuse_trivial_mask(forms, who + ": --guide-mask")
    return feather, forms


def load_guide_frames(who, path):
    """The guide's frames as a host array uint8 [N,H,W,3] (datasets.load_frames; an array [H,W,3] is one frame); anything else ends
    the program."""
    try:
        ra = datasets.load_frames(path)
    except (OSError, NotImplementedError, ValueError) as e:
        raise SystemExit("{}: --guide {}: {}".format(who, path, e))
    if ra.ndim == 3:
        ra = ra[None]
    if ra.dtype != np.uint8 or ra.ndim != 4 or ra.shape[-1] != 3 or min(ra.shape) < 1:
        raise SystemExit("{}: --guide must be uint8 [N,H,W,3] or [H,W,3], got {} {}".format(who, ra.dtype, ra.shape))
    return np.ascontiguousarray(ra)


# Rings (generate_patchnn --wrap, evaluate --wrap): what the two programs share.
def parse_wrap_axes(text):
    """--wrap AXES -> the ring flags (wt, wh, ww): a non-empty string of distinct letters of t, h, w.  Anything else ends the
    program."""
    if not isinstance(text, str) or not text or any(c not in "thw" for c in text) or len(set(text)) != len(text):
        raise SystemExit("--wrap takes a non-empty string of distinct letters of t, h, w (e.g. t, hw, thw), got {!r}".format(text))
    return tuple(int(c in text) for c in "thw")


def wrap_triple(wrap):
    """The ring flags as a triple of 0 / 1, or None for no ring at all (None, or all zero)."""
    if wrap is None:
        return None
    w = tuple(int(bool(e)) for e in wrap)
    if len(w) != 3:
        raise ValueError("wrap must be three flags (t, h, w), got %r" % (wrap,))
    return w if any(w) else None


def patchnn_wrap_pad(vol, patch, wrap):
    """The circular pad of a volume [T,H,W,3] (images [H,W,3]: T = 1) whose axes flagged in wrap = (wt, wh, ww) are rings: the
    first p - 1 slices appended along every ring axis, in the order t, y, x.  The dense patch grid of the result is the periodic
    grid of the volume, patch for patch (include/hpvg.h), so any search can run on it unchanged.  torch tensor, any device."""
    w = wrap_triple(wrap)
    if w is None:
        return vol
    image = vol.dim() == 3
    out = vol[None] if image else vol
    for ax in range(3):
        p = int(patch[ax])
        if w[ax] and p > 1:
            if out.shape[ax] < p:
                raise ValueError("patchnn_wrap_pad: a ring of %d is shorter than the patch side %d" % (out.shape[ax], p))
            out = torch.cat([out, out.narrow(ax, 0, p - 1)], ax)
    out = out.contiguous()
    return out[0] if image else out
