"""`python -m hp_vae_gan_amd.train_image --image-path ... --checkname ...`: train HP-VAE-GAN on one image (the reference's
train_image.py).  The trainer is programs.Program, shared with train_video: flags, run directory, scalars, previews and
the resume rule are described in programs.py."""
import sys

from .programs import train_main


def main(argv=None):
    return train_main("image", argv)


if __name__ == "__main__":
    sys.exit(main())
