"""Write tests/golden/cli_flags_baselines.json: the command-line flags of the reference's third program,
train_video_baselines.py, read with `ast` by make_cli_flags.flags_of (nothing is imported or executed; names, types,
defaults, nargs, actions and `required` only).

Run:  python tests/golden/make_cli_flags_baselines.py REFERENCE_DIR      (the reference checkout's root)

tests/test_cli_baselines.py holds the parser of hp_vae_gan_amd.train_video_baselines to this file."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_cli_flags import flags_of  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cli_flags_baselines.json")


def main(ref):
    data = {"train_video_baselines": flags_of(os.path.join(ref, "train_video_baselines.py"))}
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, {k: len(v) for k, v in data.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tests/golden/make_cli_flags_baselines.py REFERENCE_DIR")
    main(sys.argv[1])
