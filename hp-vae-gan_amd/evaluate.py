"""`python -m hp_vae_gan_amd.evaluate --exp-dir run/<clip>/<checkname>/experiment_<n>` (after `generate`), or
`--samples S.npy --real R.npy` without an experiment: patch nearest-neighbour coherence / completeness, nn_unique_frac and
diversity of the samples against the training clip, written to metrics.json (see programs.evaluate)."""
from .programs import evaluate_main, main_guard


def main(argv=None):
    return evaluate_main(argv)


if __name__ == "__main__":
    main_guard(main)
