"""The epoch loop of the four trainers (train_image_mt, train_captioning, train_txt2image, train_txt_sim) without a GPU: the
step methods are replaced on the instance by recorders, the model and the optimizer are stubs.  Every expected value is restated
here from the loop's rules -- shuffle with Random(seed + epoch), wrap-pad to the world size, stride by rank; a RuntimeError
skips the batch at world size 1 and propagates otherwise; the logged mean is the n-weighted mean of what was fed to the meter
since the previous line -- never taken from the code under test."""
import random
import re

import pytest
import torch

from imagetranslate_amd import train_captioning, train_image_mt, train_txt2image, train_txt_sim

SEED = 7
ALL = ("mt", "cap", "t2i", "sim")
RANKED = ("mt", "cap")  # the trainers that run under data parallelism; the other two refuse world_size > 1
# (name, count) in the order in which each train_epoch concatenates its batches before the shuffle
KINDS = {"mt": [("mt", 5), ("mass", 3), ("img", 2)], "cap": [("img", 4), ("mt", 2)], "t2i": [("img", 6)], "sim": [("mt", 6)]}
ODD = {"mt": [("mt", 5), ("mass", 3), ("img", 1)], "cap": [("img", 3), ("mt", 2)]}  # an odd total: two ranks need one wrapped batch
LOG = {"mt": r"\S+ \S+ step (\d+) loss (\S+) tokens/s \S+ lr 1\.00e-03", "cap": r"\S+ \S+ Epoch Step: (\d+) Loss: (\S+) Tokens per Sec: \S+ ",
       "t2i": r"\S+ \S+ Epoch Step: (\d+) Loss: (\S+) Image per Sec: \S+ ", "sim": r"\S+ \S+ Epoch Step: (\d+) Loss: (\S+) Sentences per Sec: \S+ "}
MEAN = {"mt": "%.4f", "cap": "%f", "t2i": "%f", "sim": "%f"}
BASE = {"mt": 0.5, "mass": 1.25, "img": 2.0}
COUNT = (4, 2, 8, 1, 16, 32)  # powers of two: loss / n (train_txt2image) is exact in float32


def loss_of(batch):
    return BASE[batch[0]] + 0.25 * batch[1]  # exact in float32, different for every batch of an epoch


def n_of(batch):
    return COUNT[batch[1]]


def all_batches(kinds):
    return [(name, i) for name, count in kinds for i in range(count)]


def shuffled(kinds, epoch):
    order = all_batches(kinds)
    random.Random(SEED + epoch).shuffle(order)
    return order


def shard(kinds, epoch, rank=0, world=1):
    order = shuffled(kinds, epoch)
    if world > 1:
        order = order + order[:(-len(order)) % world]
    return order[rank::world]


class Model:
    def __init__(self, rig):
        self.rig = rig

    def save(self, path):
        self.rig.events.append(("save", path, len(self.rig.visited)))

    def eval(self):
        return self

    def train(self, mode=True):
        return self


class Optimizer:
    def __init__(self):
        self.param_groups, self.zeroed = [{"lr": 1e-3}], 0

    def zero_grad(self):
        self.zeroed += 1


class Rig:
    """One trainer on stubs.  ``visited``: the batches whose step function returned, in order; ``events``: (what, ..., number of
    batches visited so far) of every model.save and every recorder around the loop; ``fail`` / ``empty`` / ``no_tokens``: batches
    whose step raises RuntimeError, returns (0.0, 0) like caption_step, or returns a loss with 0 tokens like the contrastive
    image step."""

    def __init__(self, name, monkeypatch, kinds=None, rank=0, world=1, fail=(), empty=(), no_tokens=()):
        self.name, self.kinds = name, kinds or KINDS[name]
        self.visited, self.events, self.sim_steps = [], [], []
        self.fail, self.empty, self.no_tokens = fail, empty, no_tokens
        self.optimizer = Optimizer()
        kw = dict(model=Model(self), optimizer=self.optimizer, seed=SEED)
        if name == "mt":
            t = train_image_mt.ImageMTTrainer(**kw)
            t.mt_step = t.mass_step = t.image_step = self.step
        elif name == "cap":
            monkeypatch.setattr(train_captioning, "BeamDecoder", lambda model, **kw: None)
            t = train_captioning.ImageCaptionTrainer(**kw)
            t.caption_step = t.mt_step = self.step
        elif name == "t2i":
            t = train_txt2image.Caption2ImageTrainer(caption_model=Model(self), **kw)
            t.txt2image_step = self.step
        else:
            t = train_txt_sim.SenSimTrainer(**kw)
            t.sim_step = self.sim_step
        t.rank, t.world_size = rank, world  # by attribute: no process group, no GradSync
        self.trainer = t
        self.data = {k: [(k, i) for i in range(count)] for k, count in self.kinds}

    def step(self, batch, *args, **kw):
        if batch in self.fail:
            raise RuntimeError("boom")
        self.visited.append(batch)
        if batch in self.empty:
            return 0.0, 0
        return torch.tensor(loss_of(batch)), 0 if batch in self.no_tokens else n_of(batch)

    def sim_step(self, batch, src_neg, dst_neg, step, accum=1):
        self.sim_steps.append(step)
        return self.step(batch)

    def record(self, what, result=None):
        def recorder(*args):
            self.events.append((what,) + args + (len(self.visited),))
            return result
        return recorder

    def epoch(self, log_every=10 ** 6, **kw):
        d, t = self.data, self.trainer
        if self.name == "mt":
            return t.train_epoch(mt_data=d["mt"], mass_data=d["mass"], img_data=d["img"], log_every=log_every, **kw)
        if self.name == "cap":
            return t.train_epoch(img_data=d["img"], mt_data=d["mt"], log_every=log_every, **kw)
        if self.name == "t2i":
            return t.train_epoch(d["img"], log_every=log_every, **kw)
        return t.train_epoch(d["mt"], ["src_neg"], ["dst_neg"], log_every=log_every, **kw)

    def fed(self, batch):
        """(value, weight) that the trainer feeds its meter for a counted batch."""
        loss, n = torch.tensor(loss_of(batch)), n_of(batch)
        if batch in self.empty or batch in self.no_tokens:
            return 0.0, 0
        return (float(loss / n) if self.name == "t2i" else float(loss)), n


def logged(name, out):
    return [m.groups() for m in (re.fullmatch(LOG[name], line) for line in out.splitlines()) if m]


def expected_lines(rig, counted, log_every, first_step=0):
    lines = []
    for k in range(log_every, len(counted) + 1, log_every):
        fed = [rig.fed(b) for b in counted[k - log_every:k]]
        total = sum(n for _, n in fed)
        lines.append((str(first_step + k), MEAN[rig.name] % (sum(v * n for v, n in fed) / max(total, 1))))
    return lines


# ------------------------------------------------------------------------------------------------ order
@pytest.mark.parametrize("name", ALL)
def test_visited_order_is_the_seeded_shuffle_of_the_concatenated_kinds(name, monkeypatch):
    rig = Rig(name, monkeypatch)
    total = len(all_batches(rig.kinds))
    assert rig.epoch() == total
    assert rig.visited == shuffled(rig.kinds, 0)
    assert rig.trainer.epoch == 1
    assert rig.epoch(step=total) == 2 * total
    assert rig.visited[total:] == shuffled(rig.kinds, 1) != rig.visited[:total]
    assert rig.trainer.epoch == 2


@pytest.mark.parametrize("name", RANKED)
def test_two_ranks_take_equal_shares_that_tile_the_wrap_padded_shuffle(name, monkeypatch):
    rigs = [Rig(name, monkeypatch, kinds=ODD[name], rank=r, world=2) for r in (0, 1)]
    steps = [rig.epoch() for rig in rigs]
    full = shuffled(ODD[name], 0)
    assert len(full) % 2 == 1
    assert steps[0] == steps[1] == len(rigs[0].visited) == len(rigs[1].visited) == (len(full) + 1) // 2
    merged = [rigs[k % 2].visited[k // 2] for k in range(len(full) + 1)]
    assert merged[:len(full)] == full and sorted(set(merged)) == sorted(all_batches(ODD[name]))
    assert merged[len(full):] == full[:1], "the padding is the head of the shuffled list"


# ------------------------------------------------------------------------------------------------ failing / empty batch, stop
@pytest.mark.parametrize("name", ALL)
def test_failing_batch_is_skipped_and_not_counted_in_one_process(name, monkeypatch, capsys):
    order = shuffled(KINDS[name], 0)
    rig = Rig(name, monkeypatch, fail=(order[2],))
    assert rig.epoch() == len(order) - 1
    assert rig.visited == order[:2] + order[3:]
    assert rig.optimizer.zeroed == 1
    assert [l for l in capsys.readouterr().out.splitlines() if l.startswith("skipping batch:")] == \
        ["skipping batch: RuntimeError('boom')"]


@pytest.mark.parametrize("name", RANKED)
def test_failing_batch_propagates_under_data_parallelism(name, monkeypatch, capsys):
    mine = shard(KINDS[name], 0, rank=1, world=2)
    rig = Rig(name, monkeypatch, rank=1, world=2, fail=(mine[1],))
    with pytest.raises(RuntimeError, match="boom"):
        rig.epoch()
    assert rig.visited == mine[:1] and rig.optimizer.zeroed == 0
    assert "skipping batch" not in capsys.readouterr().out


def test_empty_caption_batch_is_not_a_step_in_one_process(monkeypatch, capsys):
    order = shuffled(KINDS["cap"], 0)
    rig = Rig("cap", monkeypatch, empty=(order[1],))
    assert rig.epoch(log_every=2) == len(order) - 1
    assert rig.visited == order
    assert logged("cap", capsys.readouterr().out) == expected_lines(rig, order[:1] + order[2:], 2)


def test_empty_caption_batch_is_a_step_under_data_parallelism(monkeypatch, capsys):
    mine = shard(KINDS["cap"], 0, rank=0, world=2)
    rig = Rig("cap", monkeypatch, rank=0, world=2, empty=(mine[1],))
    assert rig.epoch(log_every=3) == len(mine) == 3  # the other rank counted its batch: so does this one
    assert logged("cap", capsys.readouterr().out) == expected_lines(rig, mine, 3)  # the mean is over the other two


def test_image_step_without_tokens_is_a_step_of_train_image_mt(monkeypatch, capsys):
    order = shuffled(KINDS["mt"], 0)
    rig = Rig("mt", monkeypatch, no_tokens=(("img", 0), ("img", 1)))  # the contrastive step: a loss, 0 tokens
    assert rig.epoch(log_every=5) == len(order) == 10
    assert logged("mt", capsys.readouterr().out) == expected_lines(rig, order, 5)


@pytest.mark.parametrize("name", ALL)
def test_max_step_stops_the_epoch(name, monkeypatch):
    rig = Rig(name, monkeypatch)
    assert rig.epoch(step=2, max_step=5) == 5
    assert rig.visited == shuffled(rig.kinds, 0)[:3]
    assert rig.epoch(step=5, max_step=5) == 5 and len(rig.visited) == 3
    assert rig.trainer.epoch == 2, "an epoch that runs no step still draws its order"


# ------------------------------------------------------------------------------------------------ log
@pytest.mark.parametrize("name", ALL)
def test_logged_line_every_log_every_steps_with_the_weighted_mean_since_the_last(name, monkeypatch, capsys):
    rig = Rig(name, monkeypatch)
    order = shuffled(rig.kinds, 0)
    first, log_every = (9, 3) if name == "mt" else (10, 2)  # ten batches / six: three lines, each over log_every steps
    assert rig.epoch(step=first, log_every=log_every) == first + len(order)
    lines = logged(name, capsys.readouterr().out)
    assert [s for s, _ in lines] == (["12", "15", "18"] if name == "mt" else ["12", "14", "16"])
    assert lines == expected_lines(rig, order, log_every, first_step=first)


@pytest.mark.parametrize("name", RANKED)
def test_only_rank_0_prints(name, monkeypatch, capsys):
    for rank, lines in ((0, 1), (1, 0)):
        rig = Rig(name, monkeypatch, rank=rank, world=2)
        rig.epoch(log_every=3)
        assert len(logged(name, capsys.readouterr().out)) == lines


# ------------------------------------------------------------------------------------------------ save / evaluate cadence
def test_train_image_mt_evaluates_on_its_cadence_and_saves_the_best(monkeypatch):
    rig = Rig("mt", monkeypatch)
    losses = iter([2.0, 3.0])
    rig.trainer.dev_loss = lambda dev: rig.record("dev")(dev) or next(losses)
    rig.epoch(dev_data=["dev"], eval_every=4, save_path="best")
    assert rig.events == [("dev", ["dev"], 4), ("save", "best", 4), ("dev", ["dev"], 8)]
    assert rig.trainer.best_loss == 2.0
    rig.events.clear()
    rig.epoch(step=10, dev_data=None, eval_every=4, save_path="best")
    assert rig.events == [], "no dev set: nothing is evaluated or saved inside the epoch"


def test_captioning_validates_on_its_cadence_even_without_a_dev_set(monkeypatch):
    rig = Rig("cap", monkeypatch)
    rig.trainer._validate = rig.record("validate")
    rig.epoch(eval_every=2, save_path="cap")
    assert rig.events == [("validate", None, None, "cap", k) for k in (2, 4, 6)]
    rig = Rig("cap", monkeypatch)
    rig.epoch(eval_every=4, save_path="cap")  # the real _validate, no dev set: the latest weights only
    assert rig.events == [("save", "cap.latest", 4)]
    rig.events.clear()
    rig.trainer.caption_dev_loss = rig.record("caption_dev", 1.5)
    rig.epoch(step=6, eval_every=8, save_path="cap", img_dev_data=["dev"])
    assert rig.events == [("caption_dev", ["dev"], 8), ("save", "cap.latest", 8), ("save", "cap", 8)]


def test_txt2image_saves_latest_then_prints_the_dev_loss(monkeypatch, capsys):
    rig = Rig("t2i", monkeypatch)
    rig.trainer.dev_loss = rig.record("dev", 1.5)
    rig.epoch(save_every=2, eval_every=4, save_path="m", img_dev_data=["dev"])
    assert rig.events == [("save", "m.latest", 2), ("save", "m.latest", 4), ("dev", ["dev"], 4), ("save", "m.latest", 6)]
    assert capsys.readouterr().out.splitlines() == ["Dev Loss: 1.5"]
    rig.events.clear()
    rig.epoch(step=6, save_every=2, eval_every=4)
    assert rig.events == [], "no path, no dev set: nothing is saved or evaluated"


def test_txt_sim_saves_latest_then_validates_and_saves_the_best(monkeypatch):
    rig = Rig("sim", monkeypatch)
    rig.trainer.dev_loss = rig.record("dev", 2.0)
    rig.epoch(save_every=2, eval_every=4, save_path="m", dev_data=["dev"])
    assert rig.events == [("save", "m.latest", 2), ("save", "m.latest", 4), ("dev", ["dev"], 4), ("save", "m", 4),
                          ("save", "m.latest", 6)]
    rig = Rig("sim", monkeypatch)
    rig.trainer.validate_and_save = rig.record("validate")
    rig.epoch(save_every=4, eval_every=3, save_path="m", dev_data=["dev"])
    assert rig.events == [("validate", ["dev"], "m", 3), ("save", "m.latest", 4), ("validate", ["dev"], "m", 6)]


def test_sim_step_receives_the_step_before_it_is_counted(monkeypatch):
    order = shuffled(KINDS["sim"], 0)
    rig = Rig("sim", monkeypatch, fail=(order[1],))
    assert rig.epoch(step=3) == 3 + 5
    assert rig.sim_steps == [3, 4, 4, 5, 6, 7], "draw_negative(seed, step, ...): a skipped batch does not advance the step"


# ------------------------------------------------------------------------------------------------ what the trainers are
def test_single_process_trainers_carry_no_mt_state(monkeypatch):
    for name in ("t2i", "sim"):
        t = Rig(name, monkeypatch).trainer
        assert not isinstance(t, train_image_mt.ImageMTTrainer)
        for attr in ("_mass_rng", "_img_rng", "bt_kw", "mm_mode", "mass_step", "bt_step", "image_step"):
            assert not hasattr(t, attr), (name, attr)
        for attr in ("model", "optimizer", "clip", "rank", "world_size", "sync", "best_loss", "seed", "epoch", "micro_step"):
            assert hasattr(t, attr), (name, attr)
