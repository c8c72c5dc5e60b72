"""Write tests/golden/cli_flags.json: the command-line flags of the reference's two programs (train_video.py and
train_image.py), read with `ast` from their `parser.add_argument(...)` calls - nothing is imported or executed, and only
names, types, defaults, nargs, actions and `required` are kept (no help text, no code).

Run:  python tests/golden/make_cli_flags.py REFERENCE_DIR      (build container only; the reference checkout's root)

tests/test_cli_programs.py holds the parsers of hp_vae_gan_amd.train_video / train_image to this file."""
import ast
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cli_flags.json")
PROGRAMS = {"train_video": "train_video.py", "train_image": "train_image.py"}


def _literal(node):
    if isinstance(node, ast.Name):      # type=int / float / str
        return node.id
    return ast.literal_eval(node)


def flags_of(path):
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    flags = []
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument"):
            continue
        names = [ast.literal_eval(a) for a in node.args]
        kw = {k.arg: k.value for k in node.keywords}
        entry = {"names": names, "dest": names[0].lstrip("-").replace("-", "_")}
        for key in ("type", "default", "required", "action", "nargs"):
            if key in kw:
                entry[key] = _literal(kw[key])
        flags.append((node.lineno, entry))
    return [e for _, e in sorted(flags, key=lambda t: t[0])]


def main(ref):
    data = {name: flags_of(os.path.join(ref, rel)) for name, rel in PROGRAMS.items()}
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, {k: len(v) for k, v in data.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tests/golden/make_cli_flags.py REFERENCE_DIR")
    main(sys.argv[1])
