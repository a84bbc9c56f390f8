"""What the four training entry points share (train_image_mt, train_captioning, train_txt2image, train_txt_sim): ``Trainer``
with the state every trainer keeps, the tail of a micro-step, the epoch's batch order and the one epoch loop; ``LossMeter``;
and what the ``train()`` drivers do alike around it (process group, refused flags, --dict, batch directories).  What belongs to
one model -- its step methods, its dev loss, when it saves and evaluates -- stays with that model's trainer.

A run can be interrupted and picked up again (--save-state / --resume DIR, ``add_resume_options``): ``Trainer.state_dict()`` /
``load_state_dict()`` hold the counters (step, epoch, position in the epoch's order, micro-step, best loss) and this rank's random
streams, ``run_epoch(start=...)`` enters an epoch in the middle, and with ``enable_snapshots`` the loop writes
``<model>.latest/train_state.pt`` (checkpoint.py) every --save-steps counted steps -- never inside an open accumulation window."""
import datetime
import os
import random

import torch

from . import dataset
from .parallel import GradSync, finish_micro_step


class Trainer:
    unit = "Tokens"  # what the step functions count and ``log_line`` reports per second

    def __init__(self, model, optimizer=None, clip: float = 1.0, rank: int = 0, world_size: int = 1, seed: int = 1234):
        self.model = model
        self.optimizer = optimizer
        self.clip = clip
        self.rank, self.world_size = rank, world_size
        self.sync = GradSync(model) if world_size > 1 else None
        self.best_loss = float("inf")
        self.seed = seed
        self.epoch = 0
        self.micro_step = 0  # backward passes so far: the optimizer steps when this reaches a multiple of `accum`
        self.step = 0        # counted steps so far (run_epoch keeps it)
        self.epoch_pos = 0   # index into this rank's epoch_order of the next batch to visit (run_epoch keeps it)
        self._resume_pos = None   # epoch_pos of a loaded snapshot, until the interrupted epoch is entered again
        self._datasets = []       # datasets with a generator of their own (ImageCaptionDataset._neg_rng), in order of first use
        self._pending_neg = []    # their saved states, until the trainer is handed them
        self._snapshots = None    # (directory, save_steps, accum) with state saving on
        self._snapshot_due = False
        self._latest_saved = None  # (directory, step, micro-step) of the last save_latest: a snapshot of the same moment reuses it

    def _proposals(self, batch):
        """batch["proposal"] ([B, Pmax], built by the datasets from --dict) when the model attends over proposals."""
        return batch.get("proposal") if getattr(self.model, "use_proposals", False) else None

    def _finish_micro_step(self, accum: int):
        """clip after EVERY backward, step every `accum` (src/train_image_mt.py:291-295)."""
        self.micro_step += 1
        finish_micro_step(self.model, self.optimizer, self.sync, self.clip, update=self.micro_step % max(1, accum) == 0)

    def epoch_order(self, kinds):
        """This rank's share of the epoch's batches, as (name, index) over ``kinds`` = [(name, count), ...]: the same shuffle on
        every rank (a generator seeded with seed + epoch, nothing else draws from it), padded by wrapping around to a multiple
        of the world size like torch's DistributedSampler (src/train_image_mt.py:586-589), then strided -- every rank runs the
        SAME number of steps, so no rank is left waiting in an all-reduce when an epoch ends."""
        order = [(name, i) for name, count in kinds for i in range(count)]
        random.Random(self.seed + self.epoch).shuffle(order)
        if self.world_size > 1:
            order = order + order[:(-len(order)) % self.world_size]
        return order[self.rank::self.world_size]

    def run_epoch(self, order, step_fn, *, step: int, max_step: int, log_every: int, after_step=None, skip_empty: bool = False,
                  start: int = 0):
        """One epoch over ``order[start:]`` (from ``epoch_order``), until ``max_step``; returns the step count.  ``step_fn(kind, i,
        step)`` runs one batch and returns (loss, n): what the meter is fed and its weight.  ``after_step(step)`` follows the log
        block of every counted step (saving, evaluating), then a snapshot that is due is written.  ``skip_empty``: a batch with
        n == 0 is not a step in a one-process job.  ``self.epoch_pos`` is the index of the next entry of ``order`` at every
        moment: it advances past a skipped failing batch and past a skipped empty batch too."""
        self.epoch += 1
        self.step, self.epoch_pos = step, start
        meter, t0 = LossMeter(), datetime.datetime.now()
        for pos in range(start, len(order)):
            kind, i = order[pos]
            if step >= max_step:
                break
            self.epoch_pos = pos + 1
            try:
                loss, n = step_fn(kind, i, step)
            except RuntimeError as err:  # the reference trainer skips a failing batch and goes on (src/train_image_mt.py:327-333)
                if self.world_size > 1:
                    raise  # the other ranks are inside this step's collectives: skipping here would leave them hanging
                print("skipping batch:", repr(err))
                self.optimizer.zero_grad()
                continue
            if skip_empty and n == 0 and self.world_size == 1:
                continue
            step += 1  # (an empty batch of a multi-rank job counts: the other ranks counted theirs)
            self.step = step
            meter.add(loss, n)
            if step % log_every == 0:
                mean, count = meter.read()  # the only host read of the losses: once per log_every steps, on every rank
                if self.rank == 0:
                    secs = (datetime.datetime.now() - t0).total_seconds()
                    print(datetime.datetime.now(), self.log_line(step, mean, count, secs), flush=True)
                t0 = datetime.datetime.now()
            if after_step is not None:
                after_step(step)
            if self._snapshots is not None:
                self.snapshot_if_due(step % self._snapshots[1] == 0)
        return step

    # ------------------------------------------------------------------ state that travels (checkpoint.py)
    def take_resume_pos(self) -> int:
        """Where the epoch about to begin starts: 0, or -- once after a snapshot was loaded -- the saved ``epoch_pos``, with the
        epoch counter set back so that ``epoch_order`` draws the interrupted epoch's order again.  Every ``train_epoch`` calls
        this before ``epoch_order``."""
        pos, self._resume_pos = self._resume_pos, None
        if pos is None or self.epoch == 0:
            return 0
        self.epoch -= 1
        return pos

    @property
    def epochs_begun(self) -> int:
        """Epochs begun so far, not counting one that a loaded snapshot interrupted and ``take_resume_pos`` will begin again."""
        return self.epoch - (1 if self._resume_pos is not None and self.epoch > 0 else 0)

    def drop_resume_pos(self):
        """A new phase begins with a fresh epoch: a position loaded from a snapshot that was taken on the last step of the phase
        before belongs to an epoch that is not entered again.  The epoch counter stays (the uninterrupted run's is the same)."""
        self._resume_pos = None

    def track_dataset(self, data):
        """``data`` is about to be trained or evaluated on: a dataset that draws from a generator of its own
        (ImageCaptionDataset._neg_rng) is remembered, so that the generator's state is saved, and gets the state a loaded
        snapshot holds for it.  Datasets are matched by the order in which the trainer first meets them."""
        if data is None or not hasattr(data, "_neg_rng") or any(d is data for d in self._datasets):
            return
        self._datasets.append(data)
        k = len(self._datasets) - 1
        if k < len(self._pending_neg) and self._pending_neg[k] is not None:
            data._neg_rng.setstate(unpack_random_state(self._pending_neg[k]))
            self._pending_neg[k] = None

    def rank_state(self) -> dict:
        """This rank's random streams: torch's default CPU generator (``dropout_seed`` draws from it), Python's global ``random``
        (the trainers seed it, the host ``mass_mask`` reads it) and ``_neg_rng`` of every dataset handed to the trainer."""
        neg = [pack_random_state(d._neg_rng.getstate()) for d in self._datasets]
        return {"torch": torch.get_rng_state().clone(), "python": pack_random_state(random.getstate()),
                "neg_rng": neg + [s for s in self._pending_neg[len(neg):]]}

    def load_rank_state(self, state: dict):
        torch.set_rng_state(state["torch"].cpu().to(torch.uint8))
        random.setstate(unpack_random_state(state["python"]))
        self._pending_neg = list(state.get("neg_rng", []))
        for k, d in enumerate(self._datasets):
            if k < len(self._pending_neg) and self._pending_neg[k] is not None:
                d._neg_rng.setstate(unpack_random_state(self._pending_neg[k]))
                self._pending_neg[k] = None

    def state_dict(self) -> dict:
        """Where the run stands, as plain values (``torch.load(weights_only=True)`` reads them back); ``"rank"`` holds what
        differs between the ranks (``rank_state``), everything else is the same on all of them."""
        return {"step": int(self.step), "epoch": int(self.epoch), "epoch_pos": int(self.epoch_pos), "micro_step": int(self.micro_step),
                "best_loss": float(self.best_loss), "seed": int(self.seed), "world_size": int(self.world_size),
                "rank": self.rank_state()}

    def load_state_dict(self, state: dict):
        if int(state["world_size"]) != int(self.world_size):
            raise ValueError("the snapshot was taken with world_size %d, this run has world_size %d (resuming at another world "
                             "size is not built)" % (int(state["world_size"]), int(self.world_size)))
        self.step, self.epoch, self.micro_step = int(state["step"]), int(state["epoch"]), int(state["micro_step"])
        self.epoch_pos = self._resume_pos = int(state["epoch_pos"])
        self.best_loss, self.seed = float(state["best_loss"]), int(state["seed"])  # the seed decides the epochs' orders
        self.load_rank_state(state["rank"])

    # ------------------------------------------------------------------ snapshots (--save-state)
    def enable_snapshots(self, directory: str, save_steps: int, accum: int = 1):
        """State saving on: a snapshot (the model's own ``save()`` output, then ``train_state.pt``) goes to ``directory`` every
        ``save_steps`` counted steps and at ``finish_snapshots``."""
        self._snapshots = (directory, max(1, int(save_steps)), max(1, int(accum)))

    def snapshot_if_due(self, due: bool = False) -> bool:
        """Write the snapshot that is due -- unless an accumulation window is open (``micro_step % accum != 0``): the flat
        gradient then holds a partial sum that no snapshot stores, and the write is deferred to the step that closes it."""
        self._snapshot_due = self._snapshot_due or due
        directory, _, accum = self._snapshots
        if not self._snapshot_due or self.micro_step % accum != 0:
            return False
        from .checkpoint import STATE_FILE, save_train_state
        if self._latest_saved != (directory, self.step, self.micro_step):  # (else the trainer's own write of this step stands)
            self.save_latest(directory=directory)
        save_train_state(os.path.join(directory, STATE_FILE), self)  # every rank: the ranks' streams are gathered
        self._snapshot_due = False
        return True

    def save_latest(self, save_path: str = None, directory: str = None):
        """The model's own ``save()`` output to ``<save_path>.latest`` (rank 0 writes).  With state saving on, the snapshot that
        falls due at the same step adds ``train_state.pt`` to this write instead of saving the weights again."""
        directory = directory or save_path + ".latest"
        if self.rank == 0:
            self.model.save(directory)
        self._latest_saved = (directory, self.step, self.micro_step)

    def finish_snapshots(self):
        """End of training.  With the accumulation window open nothing is written: the last snapshot stays the resume point."""
        if self._snapshots is not None and not self.snapshot_if_due(True) and self.rank == 0:
            print("no final snapshot: an accumulation window is open (micro-step %d)" % self.micro_step, flush=True)
        self._snapshot_due = False

    def begin_run(self, options, resume_dir=None) -> int:
        """What a ``train()`` driver does between building its data and its first epoch: --save-state turns snapshots to
        ``<model>.latest`` on, --resume DIR loads DIR's.  Returns the step count to start from.  The flags are read with
        ``getattr``: options parsed without ``add_resume_options`` leave both off."""
        if getattr(options, "save_state", False) and options.model_path:
            self.enable_snapshots(options.model_path + ".latest", options.save_steps, options.accum)
        if resume_dir:  # last: nothing after this point draws from a restored stream before the loop does
            self.resume(resume_dir)
            if self.rank == 0:
                print("resumed", resume_dir, "at step", self.step, "epoch", self.epoch, "position", self.epoch_pos, flush=True)
        return self.step

    def resume(self, directory: str):
        """--resume DIR: load DIR/train_state.pt into this trainer, its model and its optimizer."""
        from .checkpoint import STATE_FILE, load_train_state
        return load_train_state(os.path.join(directory, STATE_FILE), self)

    def log_line(self, step: int, mean: float, count: int, secs: float) -> str:
        return "Epoch Step: %d Loss: %f %s per Sec: %f " % (step, mean, self.unit, count / max(secs, 1e-9))


class LossMeter:
    """Token-weighted running mean of per-step losses that stay on the device until ``read()`` (the reference reads
    ``loss.item()`` every step, src/train_image_mt.py:284: a host stall per step that lets the GPU idle while the host
    prepares the next batch)."""

    def __init__(self):
        self.items = []

    def add(self, loss, n: int):
        if n:
            self.items.append((loss, int(n)))

    def read(self):
        tokens = sum(n for _, n in self.items)
        total = sum(float(l) * n for l, n in self.items)
        self.items = []
        return total / max(tokens, 1), tokens


def pack_random_state(state):
    """``random.Random.getstate()`` as plain ints: [version, [625 ints], gauss_next]."""
    version, words, gauss = state
    return [int(version), [int(w) for w in words], None if gauss is None else float(gauss)]


def unpack_random_state(packed):
    version, words, gauss = packed
    return (int(version), tuple(int(w) for w in words), None if gauss is None else float(gauss))


def add_resume_options(parser):
    """--save-state / --resume on top of an entry point's parser (they are no flags of the reference)."""
    parser.add_option("--save-state", action="store_true", dest="save_state", default=False,
                      help="write <model>.latest/train_state.pt (weights, Adam moments, trainer state) every --save-steps steps")
    parser.add_option("--resume", dest="resume_dir", metavar="DIR", default=None,
                      help="continue the run whose train_state.pt is in DIR (a <model>.latest directory)")
    return parser


def resume_dir_of(options):
    """--resume DIR, checked against --pretrained: the model is built from DIR, so another --pretrained is a contradiction."""
    directory = getattr(options, "resume_dir", None)
    if not directory:
        return None
    pre = getattr(options, "pretrained_path", None)
    if pre and os.path.realpath(pre) != os.path.realpath(directory):
        raise ValueError("--resume %s with --pretrained %s: the resumed model is built from the --resume directory" % (directory, pre))
    from .checkpoint import STATE_FILE
    if not os.path.isfile(os.path.join(directory, STATE_FILE)):
        raise FileNotFoundError("--resume %s: no %s there" % (directory, STATE_FILE))
    return directory


def init_distributed():
    """One process per GPU (src/utils.py:93-97, src/train_image_mt.py:72-76); backend "nccl" is RCCL on ROCm."""
    rank, world = 0, 1
    if "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if not dist.is_initialized():
            dist.init_process_group("nccl")
        rank, world = dist.get_rank(), dist.get_world_size()
    return rank, world


def reject_off_path(options, lm_supported: bool = False, dict_supported: bool = False):
    """Flags whose feature is not built are refused, never silently ignored: a requested pretrained initialisation or a
    resumed optimizer that quietly trains from scratch is worse than an error.  ``dict_supported``: the entry point builds a
    model that attends over lexical proposals and feeds it from the dictionary (train_image_mt, train_captioning)."""
    for flag, val in (("--dict", None if dict_supported else options.dict_path),):
        if val:
            raise NotImplementedError("%s: this entry point does not train with lexical proposals (train_image_mt and "
                                      "train_captioning do, DESIGN section 6)" % flag)
    for flag, val in (("--lm", None if lm_supported else options.lm_path), ("--cont", options.continue_train), ("--save-opt", options.save_opt)):
        if val:
            raise NotImplementedError("%s: not implemented by this trainer (masked-LM initialisation / pickled-optimizer resume, "
                                      "src/train_image_mt.py:319-321,449-462); use --pretrained to continue from saved weights, or --save-state / "
                                      "--resume to continue a run with its optimizer state" % flag)


def load_lex_dict(options):
    """--dict FILE (src/train_image_mt.py:430-432): {source word id: [proposed ids]}, or None without the flag."""
    return dataset.get_lex_dict(options.dict_path) if getattr(options, "dict_path", None) else None


def use_lex_dict(model, lex_dict, what: str):
    """The dictionary the data is built with: ``lex_dict`` for a model that attends over proposals, None otherwise.  A
    checkpoint and a --dict flag that disagree are an error, not a silent choice."""
    if bool(getattr(model, "use_proposals", False)) != (lex_dict is not None):
        raise ValueError("%s: the model was %s lexical proposals but --dict is %s" % (
            what, "built with" if model.use_proposals else "built without", "given" if lex_dict is not None else "missing"))
    return lex_dict


def batches_from(paths, cls=dataset.MTDataset, **kw):
    """The batches of ``cls(batch_pickle_dir=DIR, **kw)`` for every DIR of the comma-separated ``paths``, in that order; an
    empty list when there is none."""
    return [b for p in (paths or "").split(",") if p.strip() for b in cls(batch_pickle_dir=p.strip(), **kw).batches]
