"""`python -m hp_vae_gan_amd.generate --exp-dir run/<clip>/<checkname>/experiment_<n> --num-samples N`: sample videos
(or images) from a trained experiment; writes samples.npy and one GIF / PNG per sample (see programs.generate)."""
from .programs import generate_main, main_guard


def main(argv=None):
    return generate_main(argv)


if __name__ == "__main__":
    main_guard(main)
