"""`python -m hp_vae_gan_amd.train_video_baselines --video-path ... --checkname ...`: train a SinGAN-3D baseline on one video
(the reference's train_video_baselines.py; generator GeneratorCSG by default, GeneratorSG on request).

Flags: the reference's (train_video_baselines.py:217-272; --netD and --mode are accepted and unused, as there) plus --run-dir
and --no-hip-graph.  Setup, run directory, logbook, opt.json (with "program": "train_video_baselines", which `generate`
reads), the stage plan and the --netG resume rule are train_video's (programs.py).  Per stage (train_video_baselines.py:24-213):
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
from .programs import baseline_main, main_guard


def main(argv=None):
    return baseline_main(argv)


if __name__ == "__main__":
    main_guard(main)
