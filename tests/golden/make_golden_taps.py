"""Generate the --ker-size 5 / 7 step fixtures under tests/golden/ by IMPORTING THE REFERENCE through make_golden.py
(build container only; never runs on the GPU box).

Run:  python tests/golden/make_golden_taps.py [fixture-name ...]        (default: all four)

Each fixture is make_golden.run_stage_steps() with make_opt(ker_size=K, padd_size=K // 2) and carries the spreads that
make_golden.main() attaches to step fixtures, built the same way: the same draw once more on 8 threads with oneDNN switched
off, once with the input clip perturbed by 2^-20, and once with gradient noise of 1e-5 ahead of the optimizer steps.  The
channel widths (nfc = latent_dim) are chosen per fixture so that every file stays below 1 MiB: a 5x5x5 weight is 4.6 times a
3x3x3 one, and a fixture holds every weight four times (initial, gradient, after the step, per network).

Only DATA is written (inputs + expected outputs, as torch tensors / python scalars); no reference source text."""
import io
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

LIMIT = 1 << 20   # bytes per committed file

# name: (dims, ker_size, scale_idx, vae_levels, nfc = latent_dim, seed)
FIXTURES = {
    'taps5_3d_gan_s3.pt': (3, 5, 3, 2, 2, 120),
    'taps5_3d_vae_s1.pt': (3, 5, 1, 2, 4, 121),
    'taps5_2d_gan_s2.pt': (2, 5, 2, 1, 8, 122),
    'taps7_2d_gan_s2.pt': (2, 7, 2, 1, 6, 123),
}


def build(name, refs):
    images, n3, n2, losses, mutils = refs
    dims, K, scale_idx, vae_levels, nfc, seed = FIXTURES[name]
    nets = n3 if dims == 3 else n2

    def run():
        opt = mg.make_opt(ker_size=K, padd_size=K // 2, vae_levels=vae_levels, nfc=nfc, latent_dim=nfc)
        return mg.run_stage_steps(images, nets, losses, mutils, opt, dims, scale_idx, 1, seed=seed)

    torch.set_num_threads(1)
    fx = run()
    torch.set_num_threads(8)
    try:
        with torch.backends.mkldnn.flags(enabled=False):   # ATen's native conv kernels: another summation order
            fx8 = run()
    finally:
        torch.set_num_threads(1)
    mg.INPUT_EPS[0] = 2.0 ** -20
    try:
        fxp = run()
    finally:
        mg.INPUT_EPS[0] = 0.0
    mg.GRAD_NOISE[0] = 1e-5
    try:
        fxn = run()
    finally:
        mg.GRAD_NOISE[0] = 0.0
    fx['spread'] = [mg.merge_spread(mg.merge_spread(mg.iter_spread(a, b), mg.iter_spread(a, c)), mg.iter_spread(a, d))
                    for a, b, c, d in zip(fx['iters'], fx8['iters'], fxp['iters'], fxn['iters'])]
    return fx


def main():
    refs = mg.load_reference()
    for name in sys.argv[1:] or list(FIXTURES):
        fx = build(name, refs)
        buf = io.BytesIO()
        torch.save(fx, buf)
        size = buf.getbuffer().nbytes
        print(name, size, 'kink margin %.3g' % fx['kink_margin'])
        if size > LIMIT:
            raise SystemExit('%s: %d bytes > %d - lower its nfc in FIXTURES (nothing written)' % (name, size, LIMIT))
        with open(os.path.join(HERE, name), 'wb') as f:
            f.write(buf.getbuffer())


if __name__ == '__main__':
    main()
