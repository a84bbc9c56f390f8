"""Resume without a GPU: the epoch loop's arithmetic when it starts in the middle, the optimizer's state on a CPU flat store,
the snapshot file's refusals, its atomic write, the deferral of a snapshot past an open accumulation window, the stored form
of a Python generator, the boundary between the two phases of train_image_mt, the datasets' own generators, and each of the four
trainers' own epoch when it is entered in the middle.  The models are small nn.Modules on the CPU (no kernel runs: nothing here takes an optimizer step)."""
import io
import os
import random
import types

import pytest
import torch
import torch.nn as nn

from imagetranslate_amd import checkpoint, train_image_mt
from imagetranslate_amd.param_store import store_of
from imagetranslate_amd.trainer import Trainer, pack_random_state, reject_off_path, unpack_random_state
from imagetranslate_amd.utils import AdamInverseSqrtWithWarmup

SEED = 11
KINDS = [("mt", 3), ("mass", 2), ("img", 2)]  # 7 batches of mixed kinds
EPOCHS = 2


def through_file(obj):
    """``obj`` as ``torch.load(weights_only=True)`` gives it back: fails if it holds anything that loader rejects."""
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


# ------------------------------------------------------------------------------------------------ G. loop arithmetic
class StubOptimizer:
    def __init__(self):
        self.param_groups = [{"lr": 1e-3, "num_updates": 0}]

    def zero_grad(self):
        pass


class LoopRig:
    """The base Trainer on a fake step function.  ``visited``: every (kind, index) the step function was called with, failing
    ones included (a resumed run must meet those too).  A failing batch raises RuntimeError (skipped at world size 1); an empty
    batch returns n == 0 (no step and no micro-step at world size 1, both at world size 2: the rule of caption_step)."""

    def __init__(self, rank, world, fail=(), empty=(), seed=SEED):
        self.t = Trainer(None, StubOptimizer(), seed=seed)
        self.t.rank, self.t.world_size = rank, world  # by attribute: no process group
        self.fail, self.empty, self.visited = fail, empty, []

    def step_fn(self, kind, i, step):
        self.visited.append((kind, i))
        if (kind, i) in self.fail:
            raise RuntimeError("boom")
        if (kind, i) in self.empty:
            if self.t.world_size > 1:
                self.t.micro_step += 1
            return 0.0, 0
        self.t.micro_step += 1
        return torch.tensor(1.0), 4

    def drive(self, max_step):
        t, step = self.t, self.t.step
        while step < max_step and t.epochs_begun < EPOCHS:
            start = t.take_resume_pos()
            step = t.run_epoch(t.epoch_order(KINDS), self.step_fn, step=step, max_step=max_step, log_every=10 ** 6,
                               skip_empty=True, start=start)
        return step


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_resumed_loop_visits_what_the_uninterrupted_loop_visits_after_every_stop_point(rank, world, capsys):
    probe = LoopRig(rank, world)
    first_epoch = probe.t.epoch_order(KINDS)
    # in the first epoch's order: a failing batch second (one process only: it propagates under data parallelism) and an
    # empty batch last but one, so that stop points fall before, between and after them
    fail = (first_epoch[1],) if world == 1 else ()
    empty = (first_epoch[-2],)
    whole = LoopRig(rank, world, fail, empty)
    total = whole.drive(10 ** 9)
    assert whole.t.epoch == EPOCHS and total == whole.t.step
    assert len(whole.visited) == EPOCHS * len(first_epoch)
    for k in range(total + 1):
        head = LoopRig(rank, world, fail, empty)
        assert head.drive(k) == k
        state = through_file(head.t.state_dict())
        tail = LoopRig(rank, world, fail, empty, seed=SEED + 100)  # (the snapshot's seed decides the orders, not the new run's)
        tail.t.load_state_dict(state)
        assert tail.t.epoch_pos == head.t.epoch_pos
        assert tail.drive(10 ** 9) == total
        assert head.visited + tail.visited == whole.visited, k
        assert (tail.t.step, tail.t.epoch, tail.t.micro_step) == (whole.t.step, whole.t.epoch, whole.t.micro_step), k
    capsys.readouterr()


def test_epoch_pos_is_the_next_index_past_skipped_batches_too():
    rig = LoopRig(0, 1)
    order = rig.t.epoch_order(KINDS)
    rig.fail, rig.empty = (order[0],), (order[2],)
    seen = []
    rig.t.run_epoch(order, rig.step_fn, step=0, max_step=10 ** 9, log_every=10 ** 6, skip_empty=True,
                    after_step=lambda step: seen.append((step, rig.t.epoch_pos)))
    assert seen == [(1, 2), (2, 4), (3, 5), (4, 6), (5, 7)]
    rig2 = LoopRig(0, 1)
    rig2.t.run_epoch(order, rig2.step_fn, step=0, max_step=2, log_every=10 ** 6, start=3)
    assert rig2.visited == order[3:5] and rig2.t.epoch_pos == 5


def test_load_refuses_another_world_size():
    state = through_file(LoopRig(0, 2).t.state_dict())
    with pytest.raises(ValueError, match="world_size 2.*world_size 1"):
        LoopRig(0, 1).t.load_state_dict(state)


# ------------------------------------------------------------------------------------------------ models on the CPU
class Net(nn.Module):
    """Two layers whose flat layout is the reverse of ``parameters()`` when ``reverse``."""

    def __init__(self, reverse=False, out=5):
        super().__init__()
        self.a, self.b = nn.Linear(4, 3), nn.Linear(3, out)
        self.reverse, self.saved = reverse, []

    def flat_param_order(self):
        ps = list(self.parameters())
        return ps[::-1] if self.reverse else ps

    def save(self, path):
        os.makedirs(path, exist_ok=True)
        self.saved.append(path)


class Other(Net):
    pass


def optimizer_of(model, lr=2e-3, warmup=4):
    return AdamInverseSqrtWithWarmup(model.parameters(), lr=lr, betas=(0.9, 0.98), warmup_updates=warmup)


def fused_pair(reverse=False, seed=0, **kw):
    torch.manual_seed(seed)
    model = Net(reverse, **kw)
    st = store_of(model).ensure()
    opt = optimizer_of(model)
    assert opt._store() is st
    return model, st, opt


def fill_moments(st, seed):
    g = torch.Generator().manual_seed(seed)
    m, v = st.moments()
    m.copy_(torch.randn(m.shape, generator=g))
    v.copy_(torch.rand(v.shape, generator=g))


# ------------------------------------------------------------------------------------------------ H. optimizer state
def test_fused_state_dict_carries_the_moments_across_flat_layouts():
    model, st, opt = fused_pair()
    fill_moments(st, 1)
    opt.param_groups[0]["num_updates"] = 9
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3]
    for i, p in enumerate(model.parameters()):
        assert sd["state"][i]["exp_avg"].shape == p.shape
        assert torch.equal(sd["state"][i]["exp_avg"], st._view(st.exp_avg, p))
        assert sd["state"][i]["exp_avg"].data_ptr() != st._view(st.exp_avg, p).data_ptr(), "a copy, not a view"
    assert sd["param_groups"][0]["num_updates"] == 9 and sd["param_groups"][0]["params"] == [0, 1, 2, 3]
    model2, st2, opt2 = fused_pair(reverse=True, seed=5)
    assert [st.offset(p) for p in model.parameters()] != [st2.offset(p) for p in model2.parameters()]
    opt2.load_state_dict(through_file(sd))
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(st._view(st.exp_avg, p), st2._view(st2.exp_avg, q))
        assert torch.equal(st._view(st.exp_avg_sq, p), st2._view(st2.exp_avg_sq, q))
    assert opt2.param_groups[0]["num_updates"] == 9


def test_load_sets_lr_from_this_optimizers_schedule():
    model, st, opt = fused_pair()
    opt.param_groups[0]["num_updates"] = 9
    sd = opt.state_dict()
    other = AdamInverseSqrtWithWarmup(Net().parameters(), lr=5e-4, betas=(0.9, 0.98), warmup_updates=2)
    other.load_state_dict(sd)
    assert other.param_groups[0]["num_updates"] == 9
    assert other.param_groups[0]["lr"] == other.get_lr_for_step(9) == 5e-4 * 2 ** 0.5 * 9 ** -0.5
    assert other.param_groups[0]["lr"] != sd["param_groups"][0]["lr"]


def test_generic_path_state_dict_round_trip():
    torch.manual_seed(0)
    src, dst = nn.Linear(4, 3), nn.Linear(4, 3)
    a, b = optimizer_of(src), optimizer_of(dst)
    assert a._store() is None
    for p in src.parameters():
        a.state[p] = {"exp_avg": torch.randn_like(p), "exp_avg_sq": torch.rand_like(p)}
    a.param_groups[0]["num_updates"] = 3
    b.load_state_dict(through_file(a.state_dict()))
    for p, q in zip(src.parameters(), dst.parameters()):
        assert torch.equal(a.state[p]["exp_avg"], b.state[q]["exp_avg"]) and torch.equal(a.state[p]["exp_avg_sq"], b.state[q]["exp_avg_sq"])
        assert a.state[p]["exp_avg"].data_ptr() != b.state[q]["exp_avg"].data_ptr()
    assert b.param_groups[0]["num_updates"] == 3 and b.param_groups[0]["lr"] == b.get_lr_for_step(3)


def test_optimizer_refuses_other_counts_and_shapes():
    _, _, opt = fused_pair()
    sd = opt.state_dict()
    with pytest.raises(ValueError, match="4 parameters.*2"):
        optimizer_of(nn.Linear(4, 3)).load_state_dict(sd)
    _, st, wide = fused_pair(out=6)
    fill_moments(st, 2)
    with pytest.raises(ValueError, match="parameter 2 has shape"):
        opt.load_state_dict(wide.state_dict())


# ------------------------------------------------------------------------------------------------ snapshot file
def trainer_of(model, opt, **kw):
    return Trainer(model, opt, seed=kw.pop("seed", SEED), **kw)


def snapshot(tmp_path, name="train_state.pt", reverse=False, **kw):
    model, st, opt = fused_pair(reverse, **kw)
    fill_moments(st, 3)
    opt.param_groups[0]["num_updates"] = 6
    t = trainer_of(model, opt)
    t.step, t.epoch, t.epoch_pos, t.micro_step, t.best_loss = 6, 2, 3, 7, 1.25
    path = str(tmp_path / name)
    checkpoint.save_train_state(path, t, note="x")
    return path, model, st, opt, t


def test_snapshot_round_trip_on_the_cpu_restores_weights_moments_counters_and_streams(tmp_path):
    path, model, st, opt, t = snapshot(tmp_path)
    expect_py, expect_torch = [random.random() for _ in range(10)], torch.rand(10)
    blob = torch.load(path, weights_only=True)
    assert blob["layout"] == [("a.weight", [3, 4]), ("a.bias", [3]), ("b.weight", [5, 3]), ("b.bias", [5])]
    assert blob["num_updates"] == 6 and blob["model_class"] == "Net" and len(blob["ranks"]) == 1
    model2, st2, opt2 = fused_pair(reverse=True, seed=9)
    t2 = trainer_of(model2, opt2, seed=99)
    random.seed(123)
    torch.manual_seed(123)
    progress = checkpoint.load_train_state(path, t2)
    assert progress["note"] == "x" and progress["step"] == 6
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(p, q)
        assert torch.equal(st._view(st.exp_avg, p), st2._view(st2.exp_avg, q))
        assert torch.equal(st._view(st.exp_avg_sq, p), st2._view(st2.exp_avg_sq, q))
    assert (t2.step, t2.epoch, t2.epoch_pos, t2.micro_step, t2.best_loss, t2.seed) == (6, 2, 3, 7, 1.25, SEED)
    assert opt2.param_groups[0]["num_updates"] == 6 and opt2.param_groups[0]["lr"] == opt2.get_lr_for_step(6)
    assert st2._shadow_stale, "the bf16 shadow is rebuilt before the next forward"
    assert [random.random() for _ in range(10)] == expect_py and torch.equal(torch.rand(10), expect_torch)


# ------------------------------------------------------------------------------------------------ I. refusals
def test_load_names_the_first_layout_mismatch(tmp_path):
    path = snapshot(tmp_path)[0]
    model, _, opt = fused_pair(out=6)
    with pytest.raises(ValueError, match=r"layout entry b\.weight is \(5, 3\) in the snapshot, \(6, 3\) in this model"):
        checkpoint.load_train_state(path, trainer_of(model, opt))  # (b.bias differs too: the first one is named)
    torch.manual_seed(0)
    renamed = Net()
    renamed.c = renamed.b
    del renamed.b
    store_of(renamed).ensure()
    with pytest.raises(ValueError, match=r"layout entry b\.weight \(5, 3\) of the snapshot is no parameter of this model"):
        checkpoint.load_train_state(path, trainer_of(renamed, optimizer_of(renamed)))
    torch.manual_seed(0)
    more = Net()
    more.c = nn.Linear(2, 2)
    store_of(more).ensure()
    with pytest.raises(ValueError, match=r"parameter c\.weight \(2, 2\) of this model is no layout entry of the snapshot"):
        checkpoint.load_train_state(path, trainer_of(more, optimizer_of(more)))


def test_load_refuses_unknown_format_version_and_another_model_class(tmp_path):
    path, model, st, opt, t = snapshot(tmp_path)
    before = [p.detach().clone() for p in model.parameters()]
    blob = torch.load(path, weights_only=True)
    blob["format_version"] = 99
    torch.save(blob, path + ".v99")
    with pytest.raises(ValueError, match="format_version 99"):
        checkpoint.load_train_state(path + ".v99", t)
    torch.manual_seed(0)
    other = Other()
    store_of(other).ensure()
    with pytest.raises(ValueError, match="snapshot of a Net model.*Other"):
        checkpoint.load_train_state(path, trainer_of(other, optimizer_of(other)))
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))


def test_resume_with_a_conflicting_pretrained_is_an_error(tmp_path):
    latest, elsewhere = tmp_path / "m.latest", tmp_path / "elsewhere"
    latest.mkdir()
    elsewhere.mkdir()
    (latest / "train_state.pt").write_bytes(b"")
    opts, _ = train_image_mt.get_option_parser().parse_args(["--resume", str(latest), "--pretrained", str(elsewhere)])
    with pytest.raises(ValueError, match="--resume .* with --pretrained"):
        train_image_mt.train(opts)
    opts, _ = train_image_mt.get_option_parser().parse_args(["--resume", str(elsewhere)])
    with pytest.raises(FileNotFoundError, match="no train_state.pt"):
        train_image_mt.train(opts)


@pytest.mark.parametrize("flag", ["--cont", "--save-opt"])
def test_cont_and_save_opt_are_still_refused(flag):
    opts, _ = train_image_mt.get_option_parser().parse_args([flag, "--save-state"])
    with pytest.raises(NotImplementedError, match=flag):
        reject_off_path(opts, dict_supported=True)
    with pytest.raises(NotImplementedError, match=flag):
        train_image_mt.train(opts)


def test_the_two_flags_are_no_flags_of_the_shared_parser():
    from imagetranslate_amd.option_parser import get_img_options_parser
    from imagetranslate_amd import train_captioning, train_txt2image, train_txt_sim  # noqa: F401
    bare, _ = get_img_options_parser().parse_args([])
    assert not hasattr(bare, "save_state") and not hasattr(bare, "resume_dir")
    opts, _ = train_image_mt.get_option_parser().parse_args(["--save-state", "--resume", "d"])
    assert opts.save_state is True and opts.resume_dir == "d"


# ------------------------------------------------------------------------------------------------ J. atomicity
def test_a_failing_write_leaves_the_previous_snapshot_and_no_tmp_file(tmp_path, monkeypatch):
    path, model, st, opt, t = snapshot(tmp_path)
    first = open(path, "rb").read()
    real = torch.save

    def dies_midway(obj, f, *a, **kw):
        real({"half": 1}, f)  # something reached the disk ...
        raise OSError("disk full")  # ... and the writer died

    monkeypatch.setattr(checkpoint.torch, "save", dies_midway)
    t.step = 12
    with pytest.raises(OSError, match="disk full"):
        checkpoint.save_train_state(path, t)
    monkeypatch.setattr(checkpoint.torch, "save", real)
    assert sorted(os.listdir(tmp_path)) == ["train_state.pt"], "no .tmp is left behind to be taken for a snapshot"
    assert open(path, "rb").read() == first
    model2, _, opt2 = fused_pair(seed=4)
    assert checkpoint.load_train_state(path, trainer_of(model2, opt2))["step"] == 6


# ------------------------------------------------------------------------------------------------ cadence and deferral
def test_a_snapshot_due_inside_an_accumulation_window_waits_for_the_step_that_closes_it(tmp_path):
    model, st, opt = fused_pair()
    t = trainer_of(model, opt)
    directory = str(tmp_path / "m.latest")
    t.enable_snapshots(directory, save_steps=3, accum=2)
    written = []

    def step_fn(kind, i, step):
        t.micro_step += 1
        return torch.tensor(1.0), 1

    def after_step(step):  # runs BEFORE the snapshot of this step: what is on disk is from earlier steps
        f = os.path.join(directory, "train_state.pt")
        written.append((step, torch.load(f, weights_only=True)["trainer"]["step"] if os.path.exists(f) else None))

    t.run_epoch(t.epoch_order(KINDS), step_fn, step=0, max_step=7, log_every=10 ** 6, after_step=after_step)
    # due at 3 (micro-step 3: window open) -> written at 4; due at 6 (micro-step 6: closed) -> written at 6
    assert written == [(1, None), (2, None), (3, None), (4, None), (5, 4), (6, 4), (7, 6)]
    assert model.saved == [directory, directory], "the model's own save() output goes to the same directory, first"
    t.finish_snapshots()  # micro-step 7: the window is open, nothing is written
    assert torch.load(os.path.join(directory, "train_state.pt"), weights_only=True)["trainer"]["micro_step"] == 6
    t.micro_step += 1
    t.step = 8
    t.finish_snapshots()
    assert torch.load(os.path.join(directory, "train_state.pt"), weights_only=True)["trainer"]["step"] == 8


def test_state_saving_is_off_by_default():
    model, st, opt = fused_pair()
    t = trainer_of(model, opt)
    t.run_epoch(t.epoch_order(KINDS), lambda kind, i, step: (torch.tensor(1.0), 1), step=0, max_step=7, log_every=10 ** 6)
    t.finish_snapshots()
    assert model.saved == []


# ------------------------------------------------------------------------------------------------ K. Python generator
def test_python_generator_round_trip_through_the_stored_form():
    rng = random.Random(5)
    rng.gauss(0, 1)  # leaves gauss_next set: the third field is a float, not None
    [rng.random() for _ in range(700)]  # past one refill of the 624-word state
    packed = pack_random_state(rng.getstate())
    assert isinstance(packed, list) and isinstance(packed[0], int) and len(packed[1]) == 625
    assert all(type(w) is int for w in packed[1]) and isinstance(packed[2], float)
    other = random.Random(0)
    other.setstate(unpack_random_state(through_file(packed)))
    assert [other.getrandbits(62) for _ in range(10)] + [other.gauss(0, 1)] == [rng.getrandbits(62) for _ in range(10)] + [rng.gauss(0, 1)]
    fresh = pack_random_state(random.Random(1).getstate())
    assert fresh[2] is None and through_file(fresh) == fresh


# ------------------------------------------------------------------------------------------------ the phase boundary
class StubModel:
    def __init__(self):
        self.saved = []

    def save(self, path):
        self.saved.append(path)

    def eval(self):
        return self

    def train(self, mode=True):
        return self


class StubSchedule(StubOptimizer):
    def reset(self):
        self.param_groups[0]["num_updates"] = 0


class PhaseRig:
    """ImageMTTrainer on stub steps, driven by train_image_mt.run_phases -- the loop of ``train()`` itself.  With ``snapshots``
    a snapshot is due after EVERY step; ``save_train_state`` is replaced by a recorder, so ``states[k]`` is what a snapshot
    written after step k holds (the trainer's state as the file gives it back, and the optimizer's update count)."""

    def __init__(self, monkeypatch, ignore_mt_mass, seed=SEED, snapshots=False):
        self.model, self.opt = StubModel(), StubSchedule()
        t = self.t = train_image_mt.ImageMTTrainer(self.model, optimizer=self.opt, seed=seed)
        self.visited, self.states = [], {}
        self.options = types.SimpleNamespace(step=6, finetune_step=6, num_epochs=40, model_path=None, log_steps=10 ** 6,
                                             eval_steps=10 ** 6, accum=1, ignore_mt_mass=ignore_mt_mass)
        self.mt, self.mass = [("mt", i) for i in range(5)], [("mass", i) for i in range(3)]  # 8 batches: step 6 is mid-epoch

        def step_as(kind):
            def step(batch, *a, **kw):
                self.visited.append((kind, batch))
                t.micro_step += 1
                self.opt.param_groups[0]["num_updates"] += 1
                return torch.tensor(1.0), 4
            return step

        t.mt_step, t.mass_step, t.bt_step = step_as("mt"), step_as("mass"), step_as("bt")
        if snapshots:
            self.states[0] = (through_file(t.state_dict()), 0)
            t.enable_snapshots("m.latest", save_steps=1)
            monkeypatch.setattr(checkpoint, "save_train_state", lambda path, trainer: self.states.__setitem__(
                trainer.step, (through_file(trainer.state_dict()), self.opt.param_groups[0]["num_updates"])))

    def load(self, saved):
        state, num_updates = saved
        self.t.load_state_dict(state)
        self.opt.param_groups[0]["num_updates"] = num_updates

    def run(self):
        return train_image_mt.run_phases(self.t, self.options, self.t.step, self.mt, self.mass, lang_directions={5: 6, 6: 5})

    def final(self):
        t = self.t
        return (t.step, t.epoch, t.micro_step, t.phase, t.phase_start_step, t.phase_epoch0, self.opt.param_groups[0]["num_updates"])


@pytest.mark.parametrize("ignore_mt_mass", [False, True])
def test_a_snapshot_of_any_step_resumes_onto_the_uninterrupted_sequence_across_the_phase_boundary(monkeypatch, ignore_mt_mass):
    whole = PhaseRig(monkeypatch, ignore_mt_mass, snapshots=True)
    assert whole.run() == 12 and sorted(whole.states) == list(range(13))
    assert {k for k, _ in whole.visited[:6]} == {"mt", "mass"} and "bt" in {k for k, _ in whole.visited[6:]}
    assert whole.states[6][0]["phase"] == "train" and 0 < whole.states[6][0]["epoch_pos"] < 8, \
        "the snapshot of step == --step is taken in the train phase, in the middle of an epoch"
    assert whole.states[7][0]["phase"] == "bt" and whole.states[7][1] == 1, "the schedule was reset when the phase began"
    for k in range(13):
        tail = PhaseRig(monkeypatch, ignore_mt_mass, seed=SEED + 50)
        tail.load(whole.states[k])
        assert tail.run() == 12
        assert tail.visited == whole.visited[k:], k
        assert tail.final() == whole.final(), k


def test_the_epoch_bound_counts_the_same_after_a_resume_at_the_phase_boundary(monkeypatch):
    def rig(**kw):
        r = PhaseRig(monkeypatch, False, **kw)
        r.options.num_epochs, r.options.finetune_step = 1, 20  # one epoch per phase: 6 steps, then the 8 batches of ONE epoch
        return r
    whole = rig(snapshots=True)
    assert whole.run() == 14
    tail = rig(seed=SEED + 50)
    tail.load(whole.states[6])
    assert tail.run() == 14 and tail.visited == whole.visited[6:]


# ------------------------------------------------------------------------------------------------ datasets' own generators
class NegData:
    """What the trainers see of an ImageCaptionDataset: batches, and a generator of its own that reading a batch draws from."""

    def __init__(self, seed, n=4):
        self._neg_rng, self.n = random.Random(seed), n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return ("img", i, self._neg_rng.getrandbits(30))


def test_dataset_generators_are_saved_and_handed_back_in_order_of_first_use():
    a = Trainer(None, StubOptimizer(), seed=SEED)
    train, dev, plain = NegData(1), NegData(2), [("mt", 0)]
    for d in (train, plain, dev, train):  # a list has no generator; a dataset met twice is tracked once
        a.track_dataset(d)
    [train[0] for _ in range(3)], [dev[0] for _ in range(5)]
    state = through_file(a.state_dict())
    assert len(state["rank"]["neg_rng"]) == 2
    expect = ([train[0] for _ in range(10)], [dev[0] for _ in range(10)])
    # the load comes BEFORE the trainer has seen its datasets: the states wait, and a snapshot taken meanwhile still holds them
    b = Trainer(None, StubOptimizer(), seed=SEED)
    b.load_state_dict(state)
    again = through_file(b.state_dict())
    assert again["rank"]["neg_rng"] == state["rank"]["neg_rng"]
    train_b, dev_b = NegData(7), NegData(8)
    b.track_dataset(train_b)
    assert [train_b[0] for _ in range(10)] == expect[0]
    mixed = through_file(b.state_dict())["rank"]["neg_rng"]  # one generator live (and advanced), one still waiting
    assert mixed[1] == state["rank"]["neg_rng"][1] and mixed[0] != state["rank"]["neg_rng"][0]
    b.track_dataset(dev_b)
    assert [dev_b[0] for _ in range(10)] == expect[1]
    # the load comes AFTER: the generators are set at once
    c = Trainer(None, StubOptimizer(), seed=SEED)
    train_c, dev_c = NegData(7), NegData(8)
    c.track_dataset(train_c)
    c.track_dataset(dev_c)
    c.load_state_dict(state)
    assert ([train_c[0] for _ in range(10)], [dev_c[0] for _ in range(10)]) == expect
    d = Trainer(None, StubOptimizer(), seed=SEED)  # a chain of resumes: the state a resumed trainer saved before it saw its data
    d.load_state_dict(again)
    dev_d = NegData(9)
    d.track_dataset(NegData(7))
    d.track_dataset(dev_d)
    assert [dev_d[0] for _ in range(10)] == expect[1]


# ------------------------------------------------------------------------------------------------ the four trainers' epochs
def epoch_rig(name, monkeypatch, seed=SEED):
    """(trainer, visited, run(max_step)) of one of the four trainers on stub steps, through its own train_epoch."""
    from imagetranslate_amd import train_captioning, train_txt2image, train_txt_sim
    model, visited = StubModel(), []
    kw = dict(model=model, optimizer=StubOptimizer(), seed=seed)

    def step(batch, *a, **k):
        visited.append(batch if isinstance(batch, tuple) else tuple(batch))
        t.micro_step += 1
        return torch.tensor(1.0), 4

    img, dev, mt = NegData(1, 5), NegData(2, 2), [("mt", i) for i in range(3)]
    if name == "mt":
        t = train_image_mt.ImageMTTrainer(**kw)
        t.mt_step = t.mass_step = t.image_step = step
        epoch = lambda s, m: t.train_epoch(mt_data=mt, mass_data=[("mass", 0), ("mass", 1)], img_data=img, step=s, max_step=m, log_every=10 ** 6)
    elif name == "cap":
        monkeypatch.setattr(train_captioning, "BeamDecoder", lambda model, **kw: None)
        t = train_captioning.ImageCaptionTrainer(**kw)
        t.caption_step = t.mt_step = step
        t._validate = lambda *a: None
        epoch = lambda s, m: t.train_epoch(img_data=img, mt_data=mt, img_dev_data=dev, step=s, max_step=m, log_every=10 ** 6)
    elif name == "t2i":
        t = train_txt2image.Caption2ImageTrainer(caption_model=StubModel(), **kw)
        t.txt2image_step = step
        t.dev_loss = lambda data: 0.0
        epoch = lambda s, m: t.train_epoch(img, img_dev_data=dev, step=s, max_step=m, log_every=10 ** 6, save_path="m", save_every=2,
                                           eval_every=10 ** 6)
    else:
        t = train_txt_sim.SenSimTrainer(**kw)
        t.sim_step = lambda batch, src_neg, dst_neg, s, accum=1: step(batch + (s,))  # the step the negatives are drawn from
        epoch = lambda s, m: t.train_epoch(mt + [("mt", 3), ("mt", 4)], ["n"], ["n"], step=s, max_step=m, log_every=10 ** 6, save_path=None)

    def run(max_step):
        s = t.step
        while s < max_step and t.epochs_begun < 2:
            s = epoch(s, max_step)
        return s

    return t, visited, run, (img, dev)


@pytest.mark.parametrize("name", ["mt", "cap", "t2i", "sim"])
def test_every_trainers_own_epoch_enters_at_the_saved_position(name, monkeypatch, capsys):
    whole_t, whole, run, _ = epoch_rig(name, monkeypatch)
    total = run(10 ** 9)
    assert total == len(whole) == 2 * {"mt": 10, "cap": 8, "t2i": 5, "sim": 5}[name] and whole_t.epoch == 2
    for k in range(total + 1):
        head_t, head, run_head, _ = epoch_rig(name, monkeypatch)
        assert run_head(k) == k
        state = through_file(head_t.state_dict())
        tail_t, tail, run_tail, data = epoch_rig(name, monkeypatch, seed=SEED + 9)
        tail_t.load_state_dict(state)
        assert run_tail(10 ** 9) == total
        assert head + tail == whole, (name, k)  # (image batches carry the draw of the dataset's generator, txt_sim's the step)
        assert (tail_t.step, tail_t.epoch, tail_t.micro_step) == (total, 2, total)
        if name in ("cap", "t2i") and k > 0:
            assert len(state["rank"]["neg_rng"]) == 2, "the dev dataset's generator is saved beside the training set's"


def test_a_snapshot_adds_train_state_to_the_latest_write_of_the_same_step(monkeypatch):
    t, visited, run, _ = epoch_rig("t2i", monkeypatch)
    written = []
    monkeypatch.setattr(checkpoint, "save_train_state", lambda path, trainer: written.append((path, trainer.step, len(trainer.model.saved))))
    t.enable_snapshots("m.latest", save_steps=2)  # the cadence of the trainer's own .latest write (save_every=2 in the rig)
    assert run(5) == 5
    assert t.model.saved == ["m.latest", "m.latest"], "steps 2 and 4: the weights are written once, not twice"
    assert written == [(os.path.join("m.latest", "train_state.pt"), 2, 1), (os.path.join("m.latest", "train_state.pt"), 4, 2)]
    t.enable_snapshots("m.latest", save_steps=3)  # another cadence: the snapshot writes the weights itself
    t.step = 6
    t.snapshot_if_due(True)
    assert t.model.saved == ["m.latest"] * 3 and written[-1][1:] == (6, 3)
