"""`python -m hp_vae_gan_amd.train_video --video-path ... --checkname ...`: train HP-VAE-GAN on one video (the reference's
train_video.py).  The trainer is programs.Program, shared with train_image: flags, run directory, scalars, previews and
the resume rule are described in programs.py."""
import sys

from .programs import train_main


def main(argv=None):
    return train_main("video", argv)


if __name__ == "__main__":
    sys.exit(main())
