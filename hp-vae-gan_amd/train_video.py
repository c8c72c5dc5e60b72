"""`python -m hp_vae_gan_amd.train_video --video-path ... --checkname ...`: train HP-VAE-GAN on one video (the reference's
train_video.py).  Flags, run directory, scalars, previews and the resume rule: see programs.py."""
from .programs import main_guard, train_main


def main(argv=None):
    return train_main("video", argv)


if __name__ == "__main__":
    main_guard(main)
