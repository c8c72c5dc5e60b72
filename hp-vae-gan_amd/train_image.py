"""`python -m hp_vae_gan_amd.train_image --image-path ... --checkname ...`: train HP-VAE-GAN on one image (the reference's
train_image.py).  Flags, run directory, scalars, previews and the resume rule: see programs.py."""
from .programs import main_guard, train_main


def main(argv=None):
    return train_main("image", argv)


if __name__ == "__main__":
    main_guard(main)
