"""`python -m hp_vae_gan_amd.train_video_baselines --video-path ... --checkname ...`: train a SinGAN-3D baseline on one video
(the reference's train_video_baselines.py; generator GeneratorCSG by default, GeneratorSG on request).

Flags: the reference's (train_video_baselines.py:217-272; --netD and --mode are accepted and unused, as there) plus --run-dir
and --no-hip-graph.  Setup, run directory, logbook, opt.json (with "program": "train_video_baselines", which `generate`
reads), the stage plan and the --netG resume rule are train_video's (programs.Program).  Per stage (train_video_baselines.py:24-213):
get_fps_td_by_index, dataset.generate_frames, Z_init on the first stage the process trains, the critic of class
--discriminator warm-started from netD_{s-1}.pth from scale 1 on, then train.train_baseline (two eager iterations, then
hipGraph replay) and the reference's checkpoints: Noise_Amps.pth, netG.pth, netD_<s>.pth and Z_init.pth.

Z_init, the fixed reconstruction noise, is drawn once per process (train_video_baselines.py:38-43), shaped
[batch, 3, td, H0, W0] with the level-0 height and width and the time depth of that first stage - on a resume the resumed
scale's - and written to Z_init.pth when drawn and at the end of every stage.  As in the reference a resume does not load
the old run's Z_init.

Deliberate divergence: on the resumed scale the critic is warm-started from the RESUME directory's netD_{s-1}.pth.  The
reference always reads its own experiment directory (train_video_baselines.py:45-48), which holds no such file after a
resume, so the reference stops there with a missing-file error.

Scalars: the loss log is drained into scalars.jsonl every --print-interval iterations and at the end of each stage, under
the reference's tags `Video/Scale {s}/errG`, `errD_fake`, `errD_real` and, when alpha > 0, `rec_loss` and `noise_amp`
(train_video_baselines.py:178-184), plus `gradient_penalty`.  Previews (--visualize) at iteration % print_interval == 0:
GIFs of that iteration's real, generated (alpha > 0) and fake (train_video_baselines.py:190-196); they draw nothing."""
import os
import sys

import torch

from . import checkpoint
from . import train as hp_train
from . import utils as hp_utils
from .modules import networks_3d
from . import snapshot
from .programs import Program, trainer_parser

# column of the baselines' loss log -> the reference's tag (train_video_baselines.py:178-184: `rec_loss`, not train_video's
# `rec loss`) or this project's own (gradient_penalty)
BASELINE_TAGS = {"errD_real": "errD_real", "errD_fake": "errD_fake", "gradient_penalty": "gradient_penalty", "errG": "errG",
                 "rec_loss": "rec_loss"}


def build_baseline_parser():
    """The reference's parser of train_video_baselines.py:217-272 (same names, types, defaults and `required`), plus --run-dir
    and --no-hip-graph."""
    p = trainer_parser("train_video_baselines", "Train a SinGAN-3D baseline on one video, stage by stage, on an MI355X.")
    a = p.add_argument
    a('--nc-z', type=int, default=3, help='noise channels')
    a('--generator', type=str, help='generator class (GeneratorCSG, GeneratorSG)', default='GeneratorCSG')
    a('--discriminator', type=str, help='discriminator class (WDiscriminator3D, WDiscriminatorBaselines)',
      default='WDiscriminator3D')
    a('--Gsteps', type=int, default=1, help='generator optimizer steps per iteration')
    a('--Dsteps', type=int, default=1, help='discriminator updates per iteration')
    a('--alpha', type=float, help='reconstruction loss weight', default=10.)
    a('--mode', default='train', help='accepted, unused (as in the reference)')
    a('--visualize', action='store_true', default=False, help='write GIF previews under previews/')
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
    """One training run of train_video_baselines (see the module docstring): programs.Program's setup and stage with the
    baselines' parser, critic, loss-log columns, train function and Z_init."""

    tags = BASELINE_TAGS
    program = 'train_video_baselines'
    train_fn = staticmethod(hp_train.train_baseline)

    def __init__(self, argv=None):
        super().__init__('video', argv)
        # only now, after opt.json is written: json_settings keeps None, so an earlier None would land there and in the logbook
        self.opt.Z_init = None   # drawn at the first stage this process trains

    def parser(self):
        return snapshot.add_flags(build_baseline_parser())

    def check_taps(self, opt):
        if opt.ker_size != 3:
            raise SystemExit("--ker-size {}: the SinGAN baselines' hard-wired pads of num_layer + 2 voxels fit ker_size=3 only "
                             "(in the reference too)".format(opt.ker_size))

    def check_flags(self, opt):
        """None of train_video's: there are no VAE levels."""

    def logs_noise_amp(self):
        return self.opt.alpha > 0   # (train_video_baselines.py:181-184)

    def save_z_init(self):
        torch.save({'data': self.opt.Z_init.detach().cpu()}, os.path.join(self.exp_dir, 'Z_init.pth'))

    def begin_stage(self):
        opt = self.opt
        if opt.Z_init is None:
            opt.Z_init = hp_utils.generate_noise(size=z_init_shape(opt), device=opt.device)
            self.save_z_init()

    def make_discriminator(self):
        opt = self.opt
        netD = getattr(networks_3d, opt.discriminator)(opt).to(opt.device)
        src = baseline_netD_dir(opt, self.exp_dir)
        if src is not None:
            checkpoint.warm_start_discriminator(netD, src, opt.scale_idx)
            self.log("Scale {}: critic warm-started from {}".format(opt.scale_idx,
                                                                   os.path.join(src, 'netD_{}.pth'.format(opt.scale_idx - 1))))
        return netD

    def loss_columns(self, netD):
        return hp_train.baseline_loss_log_columns(self.opt.alpha)

    def end_stage(self, trainer):
        self.log("Scale {}: {} iterations, hipGraph replay {}".format(
            self.opt.scale_idx, trainer.iteration, 'on' if getattr(trainer, '_graph', None) is not None else 'off'))
        self.save_z_init()

    def preview_items(self, real, out):
        """real, generated (alpha > 0) and fake of this iteration (train_video_baselines.py:190-196); no extra draws."""
        return [(name, x) for name, x in (('real', real), ('generated', out['generated']), ('fake', out['fake']))
                if x is not None]


def main(argv=None):
    BaselineProgram(argv).run()
    return 0


if __name__ == "__main__":
    sys.exit(main())
