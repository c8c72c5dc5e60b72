"""`python -m hp_vae_gan_amd.generate_patchnn --exp-dir run/<clip>/<checkname>/experiment_<n>` (or `--video-path clip.npy --out
dir`, `--image-path img.png --out dir`): training-free samples of the clip by coarse-to-fine patch nearest neighbours (GPNN /
VGPNN); writes samples.npy, one GIF / PNG per sample and patchnn.json (see programs.generate_patchnn)."""
from .programs import generate_patchnn_main, main_guard


def main(argv=None):
    return generate_patchnn_main(argv)


if __name__ == "__main__":
    main_guard(main)
