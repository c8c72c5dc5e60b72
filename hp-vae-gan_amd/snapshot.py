"""Mid-stage snapshots of a training run and their exact resume (train_video, train_image, train_video_baselines).

Flags (add_flags; the reference's parsers stay as they are): --snapshot-interval K writes <experiment>/snapshot.pth after every
K-th iteration of a stage (3 <= k < niter: under hipGraph the iterations before are the two eager ones and the capture's
warm-up, whose gradient-penalty alpha comes from another generator than every later iteration's) and at the end of every
stage; --snapshot-exit-after N ends the process cleanly after the N-th snapshot it wrote; --resume EXP_DIR continues the run
whose snapshot lies in EXP_DIR, in that directory, with every setting taken from the snapshot.

A resumed run is THE SAME run: its checkpoints and scalars.jsonl equal, bit for bit, those of the run that was never
stopped.  The resume repeats the ordinary setup from the recorded command line (same code path, same generator draws), builds
the stage the normal way, and only then puts the state back into the objects that setup made.  What a snapshot holds:

  header      format version, program, recorded command line, stage, iteration k, niter, stage_done, the interval
  networks    netG.state_dict(); netD.state_dict() inside a GAN stage (BatchNorm counts flushed; spectral-norm u / v inside)
  optimizers  inside a stage: per group the flat Adam moments m and v, and the step count (host t and device t_dev)
  trainer     opt.Noise_Amps, opt.noise_amp, the trainer's _graph_alpha, the baselines' Z_init
  random      python random, torch's CPU generator, torch's device generator, the library stream's device iteration counter
  loader      the CPU generators as they were before the current epoch's iter(loader) and the batches taken from it since
  loss log    its device cursor (the snapshot drains it first) and the byte length of scalars.jsonl
  digest      64 bits computed ON THE DEVICE from the live tensors (ops.state_digest): after a restore it is computed again
              from the live tensors and must be equal, or the resume stops - a damaged file, an arena laid out differently
              or a tensor restored into the wrong place never trains on

Written as snapshot.pth.tmp and renamed; tensors and plain python values only (torch.load(weights_only=True)).  The host-only
parts (flags, recorded command line, loader position, generator capture, scalars truncation, file round trip) need no device."""
import argparse
import os
import random

import torch

VERSION = 1
FILE = 'snapshot.pth'
PROGRAMS = ('train_video', 'train_image', 'train_video_baselines')
SKIPPABLE = frozenset(['adam', 'rng_iter', 'cuda_rng', 'loader', 'random'])   # restore()'s test hook


class ExitAfter(Exception):
    """--snapshot-exit-after: the N-th snapshot of this process is on disk."""


# ------------------------------------------------------------------------------------------------------------------ flags
def add_flags(parser):
    """The three snapshot flags, added to what build_parser / build_baseline_parser return (those hold the reference's flags
    and stay untouched)."""
    a = parser.add_argument
    a('--snapshot-interval', type=int, default=0, metavar='K',
      help='write <experiment>/snapshot.pth every K iterations of a stage and at the end of every stage (0: never)')
    a('--snapshot-exit-after', type=int, default=None, metavar='N',
      help='end the process (status 0) right after the N-th snapshot it wrote; needs --snapshot-interval')
    a('--resume', default='', metavar='EXP_DIR',
      help='continue the run whose snapshot.pth is in EXP_DIR, in that directory; every setting comes from the snapshot')
    return parser


def _flag_parser():
    p = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    add_flags(p)
    return p


def split_flags(argv):
    """(the three flags' namespace, argv without them).  --snapshot-interval is None when absent (a resume then takes the
    recorded one)."""
    p = _flag_parser()
    p.set_defaults(snapshot_interval=None)
    ns, rest = p.parse_known_args(list(argv))
    return ns, rest


def _names_flag(argv, flag):
    return any(a == flag or a.startswith(flag + '=') for a in argv)


def check_flags(ns, rest):
    """Refusals that need nothing but the command line (SystemExit)."""
    if ns.snapshot_interval is not None and ns.snapshot_interval < 0:
        raise SystemExit("--snapshot-interval: {} is negative (0 is off)".format(ns.snapshot_interval))
    if ns.snapshot_exit_after is not None:
        if ns.snapshot_exit_after < 1:
            raise SystemExit("--snapshot-exit-after: {} (1 or more snapshots)".format(ns.snapshot_exit_after))
        if not ns.resume and not ns.snapshot_interval:
            raise SystemExit("--snapshot-exit-after needs --snapshot-interval")
        if ns.resume and ns.snapshot_interval == 0:
            raise SystemExit("--snapshot-exit-after needs --snapshot-interval")
    if ns.resume:
        if _names_flag(rest, '--netG'):
            raise SystemExit("--resume continues a run from its snapshot; --netG starts another run from a finished stage: "
                             "give one of them")
        if rest:
            raise SystemExit("--resume takes every setting from the snapshot; beside it only --snapshot-interval and "
                             "--snapshot-exit-after are accepted, got: {}".format(' '.join(rest)))


def recorded_command_line(rest, seed, seed_given):
    """The command line a resume runs setup from: the run's own without the three snapshot flags, with the seed in force made
    explicit when it was drawn."""
    out = list(rest)
    if not seed_given:
        out += ['--manualSeed', str(int(seed))]
    return out


def resolve(argv, program):
    """Before the device is asked for: split and check the flags and, for --resume, load and check the snapshot.
    Returns (argv of the ordinary setup, flags namespace, snapshot dict or None)."""
    ns, rest = split_flags(argv)
    check_flags(ns, rest)
    if not ns.resume:
        ns.snapshot_interval = ns.snapshot_interval or 0
        return rest, ns, None
    snap = load(ns.resume, program)
    if ns.snapshot_interval is None:
        ns.snapshot_interval = int(snap['snapshot_interval'])
    return list(snap['argv']), ns, snap


# ------------------------------------------------------------------------------------------------------------------- file
def write(exp_dir, snap):
    """snapshot.pth.tmp, then os.replace: a reader sees the previous snapshot or this one, whole.  Returns the bytes."""
    path = os.path.join(exp_dir, FILE)
    torch.save(snap, path + '.tmp')
    size = os.path.getsize(path + '.tmp')
    os.replace(path + '.tmp', path)
    return size


def load(exp_dir, program):
    """The snapshot of exp_dir, checked for format version and program (SystemExit otherwise)."""
    path = os.path.join(exp_dir, FILE)
    if not os.path.isfile(path):
        raise SystemExit("--resume: no {} in '{}'".format(FILE, exp_dir))
    try:
        snap = torch.load(path, map_location='cpu', weights_only=True)
    except Exception as e:   # a truncated or damaged file
        raise SystemExit("--resume: {} cannot be read: {}".format(path, e))
    if not isinstance(snap, dict) or snap.get('version') != VERSION:
        raise SystemExit("--resume: {} has format version {}, this program reads version {}".format(
            path, snap.get('version') if isinstance(snap, dict) else None, VERSION))
    if snap.get('program') != program:
        raise SystemExit("--resume: {} was written by {}, not by {}".format(path, snap.get('program'), program))
    return snap


def truncate_scalars(path, length):
    """Cut scalars.jsonl back to the byte length the snapshot recorded: lines a stopped run drained after its last snapshot are
    written again by the resumed run."""
    have = os.path.getsize(path) if os.path.exists(path) else 0
    if have < length:
        raise SystemExit("--resume: {} holds {} bytes, the snapshot recorded {}".format(path, have, length))
    if have > length:
        os.truncate(path, length)


# ------------------------------------------------------------------------------------------------- generators and loader
def host_rng_state():
    """python random and torch's CPU generator, now."""
    return {'python': random.getstate(), 'torch': torch.get_rng_state()}


def _as_getstate(v):
    """random.getstate()'s nesting, as tuples (a loaded file may hand lists)."""
    return tuple(_as_getstate(e) for e in v) if isinstance(v, (list, tuple)) else v


def set_host_rng_state(st, skip=()):
    if 'random' not in skip:
        random.setstate(_as_getstate(st['python']))
    torch.set_rng_state(st['torch'])


class LoaderPosition:
    """Where a re-iterated DataLoader stands: the host generators as they were before the current epoch's iter(loader), and the
    batches taken from that epoch.  iterate() keeps it; state() / restore() move it through a snapshot."""

    def __init__(self):
        self.epoch_start = None
        self.taken = 0
        self._pending = None

    def state(self):
        return {'epoch_start': self.epoch_start, 'taken': int(self.taken)}

    def restore(self, saved, now, skip=()):
        """The next epoch iterate() starts is the saved one, continued: `saved` = state() of the snapshot, `now` = the host
        generators at the snapshot.  skip 'loader': the position is dropped (a fresh epoch; test hook)."""
        self._pending = (None if 'loader' in skip else saved, now, tuple(skip))


def iterate(loader, pos=None, holder=None):
    """One epoch of `loader`, batch by batch, as `for item in loader` yields them.  pos (LoaderPosition or None) counts the
    batches and remembers the epoch's start; after pos.restore() the epoch is the saved one from its saved position on:
    the saved start states are set, the iterator is made, the batches already used are taken and dropped, and the generators
    are set to what they were at the snapshot.  holder[0] = the batch at hand."""
    it = None
    if pos is not None:
        pending, pos._pending = pos._pending, None
        if pending is not None:
            saved, now, skip = pending
            if saved is not None and saved['epoch_start'] is not None:
                set_host_rng_state(saved['epoch_start'], skip)
                pos.epoch_start = saved['epoch_start']
                it = iter(loader)
                for _ in range(saved['taken']):
                    next(it)
                pos.taken = saved['taken']
            set_host_rng_state(now, skip)
    if it is None:
        if pos is not None:
            pos.epoch_start = host_rng_state()
            pos.taken = 0
        it = iter(loader)
    for item in it:
        if pos is not None:
            pos.taken += 1
        if holder is not None:
            holder[0] = item
        yield item


# ------------------------------------------------------------------------------------------------------------ device state
def _optimizers(trainer):
    return [(n, getattr(trainer, n)) for n in ('optimizerG', 'optimizerD') if getattr(trainer, n, None) is not None]


def digest_tensors(prog, trainer, stage_done):
    """The live device tensors the digest covers, in its order: netG's state_dict values, netD's, per optimizer and group m, v
    and the step counter, the library stream's iteration counter, the baselines' Z_init."""
    from . import ops
    opt = prog.opt
    ts = list(prog.netG.state_dict().values())
    if not stage_done:
        if trainer.netD is not None:
            ts += list(trainer.netD.state_dict().values())
        for _, o in _optimizers(trainer):
            for g in o.groups:
                ts += [g['m'], g['v']]
            ts.append(o.t_dev)
    ts.append(ops._rng(opt.device).iter_dev)
    if getattr(opt, 'Z_init', None) is not None:
        ts.append(opt.Z_init)
    return ts


def state_digest(prog, trainer, stage_done):
    from . import ops
    return ops.state_digest(digest_tensors(prog, trainer, stage_done))


def collect(prog, trainer, log, stage_done):
    """The snapshot dict of `prog` after iteration trainer.iteration of stage opt.scale_idx (stage_done: after the stage's
    checkpoints).  The caller has drained `log` and flushed scalars.jsonl."""
    from . import ops
    opt = prog.opt
    dev = opt.device
    snap = {'version': VERSION, 'program': prog.program_name(), 'argv': list(prog.recorded_argv),
            'snapshot_interval': int(prog.snap_interval), 'stage': int(opt.scale_idx), 'iteration': int(trainer.iteration),
            'niter': int(opt.niter), 'stage_done': bool(stage_done)}
    snap['netG'] = {k: v.detach().cpu() for k, v in prog.netG.state_dict().items()}
    if not stage_done:
        if trainer.netD is not None:
            snap['netD'] = {k: v.detach().cpu() for k, v in trainer.netD.state_dict().items()}
        for name, o in _optimizers(trainer):
            snap[name] = {'steps': o.steps(), 'm': [g['m'].detach().cpu() for g in o.groups],
                          'v': [g['v'].detach().cpu() for g in o.groups]}
        snap['graph_alpha'] = bool(getattr(trainer, '_graph_alpha', False))
        snap['loader'] = prog.loader_pos.state()
        snap['log_cursor'] = int(log.drained)
    snap['Noise_Amps'] = [float(a) if isinstance(a, float) else int(a) for a in opt.Noise_Amps]
    snap['noise_amp'] = float(opt.noise_amp) if isinstance(opt.noise_amp, float) else int(opt.noise_amp)
    if getattr(opt, 'Z_init', None) is not None:
        snap['Z_init'] = opt.Z_init.detach().cpu()
    snap['rng'] = dict(host_rng_state(), cuda=torch.cuda.get_rng_state(dev), lib_iter=int(ops._rng(dev).iter_dev.item()))
    snap['scalars_bytes'] = int(os.path.getsize(prog.scalars.name))
    snap['digest'] = state_digest(prog, trainer, stage_done)
    return snap


def _refuse_digest(prog, trainer, snap):
    got = state_digest(prog, trainer, snap['stage_done'])
    if got != snap['digest']:
        raise SystemExit("--resume: the restored state's digest {:016x} is not the snapshot's {:016x} (stage {}, iteration {}): "
                         "the file is damaged or the state was laid out differently; not continuing".format(
                             got, snap['digest'], snap['stage'], snap['iteration']))


def restore_settings(prog, snap):
    """Before the resumed stage is built: what setup and the earlier stages left on the blackboard."""
    opt = prog.opt
    opt.Noise_Amps = list(snap['Noise_Amps'])
    opt.noise_amp = snap['noise_amp']
    if 'Z_init' in snap:
        opt.Z_init = snap['Z_init'].to(opt.device)


def _restore_device_rng(opt, snap, skip):
    from . import ops
    if 'cuda_rng' not in skip:
        torch.cuda.set_rng_state(snap['rng']['cuda'], opt.device)
    if 'rng_iter' not in skip:
        ops._rng(opt.device).iter_dev.fill_(int(snap['rng']['lib_iter']))


def restore_finished_stage(prog, snap, skip=(), verify=True):
    """A snapshot with stage_done: the generator as the stage left it and the generators; the loop goes on with the next
    stage as the uninterrupted one does."""
    from . import ops
    prog.netG.load_state_dict(snap['netG'])
    ops.weights_changed()
    _restore_device_rng(prog.opt, snap, skip)
    set_host_rng_state(snap['rng'], skip)
    if verify:
        _refuse_digest(prog, None, snap)


def restore(prog, trainer, log, snap, skip=(), verify=True):
    """Put a mid-stage snapshot back into the stage that was just built the normal way (trainer with its arenas, `log`,
    prog.loader_pos).  skip (test hook): names of SKIPPABLE left as the fresh stage has them; verify: refuse a state whose
    digest is not the saved one."""
    from . import ops
    skip = frozenset(skip)
    assert skip <= SKIPPABLE, skip - SKIPPABLE
    opt = prog.opt
    prog.netG.load_state_dict(snap['netG'])
    if trainer.netD is not None:
        trainer.netD.load_state_dict(snap['netD'])
    for name, o in _optimizers(trainer):
        saved = snap[name]
        if len(saved['m']) != len(o.groups) or any(m.numel() != g['m'].numel() for m, g in zip(saved['m'], o.groups)):
            raise SystemExit("--resume: {} of the snapshot has other parameter groups than this stage".format(name))
        if 'adam' not in skip:
            for g, m, v in zip(o.groups, saved['m'], saved['v']):
                g['m'].copy_(m)
                g['v'].copy_(v)
        o.t = int(saved['steps'])
        o.t_dev.fill_(int(saved['steps']))
    ops.weights_changed()
    trainer._graph_alpha = bool(snap['graph_alpha'])
    trainer.iteration = int(snap['iteration'])
    trainer.resumed_at = trainer.iteration
    log.cursor.fill_(int(snap['log_cursor']))
    log.drained = int(snap['log_cursor'])
    _restore_device_rng(opt, snap, skip)
    set_host_rng_state(snap['rng'], skip)
    prog.loader_pos.restore(snap['loader'], {'python': snap['rng']['python'], 'torch': snap['rng']['torch']}, skip)
    if verify:
        _refuse_digest(prog, trainer, snap)
