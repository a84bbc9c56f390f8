"""What the four training entry points share (train_image_mt, train_captioning, train_txt2image, train_txt_sim): ``Trainer``
with the state every trainer keeps, the tail of a micro-step, the epoch's batch order and the one epoch loop; ``LossMeter``;
and what the ``train()`` drivers do alike around it (process group, refused flags, --dict, batch directories).  What belongs to
one model -- its step methods, its dev loss, when it saves and evaluates -- stays with that model's trainer."""
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

    def run_epoch(self, order, step_fn, *, step: int, max_step: int, log_every: int, after_step=None, skip_empty: bool = False):
        """One epoch over ``order`` (from ``epoch_order``), until ``max_step``; returns the step count.  ``step_fn(kind, i, step)``
        runs one batch and returns (loss, n): what the meter is fed and its weight.  ``after_step(step)`` follows the log block
        of every counted step (saving, evaluating).  ``skip_empty``: a batch with n == 0 is not a step in a one-process job."""
        self.epoch += 1
        meter, t0 = LossMeter(), datetime.datetime.now()
        for kind, i in order:
            if step >= max_step:
                break
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
            meter.add(loss, n)
            if step % log_every == 0:
                mean, count = meter.read()  # the only host read of the losses: once per log_every steps, on every rank
                if self.rank == 0:
                    secs = (datetime.datetime.now() - t0).total_seconds()
                    print(datetime.datetime.now(), self.log_line(step, mean, count, secs), flush=True)
                t0 = datetime.datetime.now()
            if after_step is not None:
                after_step(step)
        return step

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
                                      "src/train_image_mt.py:319-321,449-462); use --pretrained to continue from saved weights" % flag)


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
