"""Resume on the GPU (--save-state / --resume): a snapshot puts weights, Adam moments, counters and every random stream back
exactly (A); a run continued from a snapshot visits the batches, draws the seeds and follows the learning-rate schedule of the
uninterrupted run exactly and stays on its trajectory within the bar (B), also across an accumulation window (C), through the
command line (D), inside the back-translation phase (E) and with two ranks (F).

State and inputs are compared exactly.  Trajectories are compared at a tolerance: the training step adds with float atomics
(embedding backward, LayerNorm dgamma / dbeta, column sums, split-K), so two runs of the SAME program from the same seed need not
agree bit for bit.  Measured on the MI355X (profiles/resume_parity.json, written by tools/resume_measure.py from the functions
below; worst per-tensor rel_err over weights and both moments after the 12 toy steps):

  * the same uninterrupted run again, five repeats against the first: up to 3.0 over all tensors -- every attention KEY BIAS
    differs by more than its own size -- and 3.2e-6 to 2.7e-5 over all the others in the recorded set of repeats, 8.4e-6 to
    3.6e-5 in the one before it (the worst is always the word embeddings; the moments at most 4.4e-6 and 1.6e-6);
  * resumed against uninterrupted: 1.8 on the key biases, 2.7e-5 on the others (moments 3.3e-6 and 1.1e-6); in these tests
    6.7e-6 (B), 4.6e-5 (C, across the accumulation window) and 2.3e-6 (F, two ranks);
  * the weights-only control against uninterrupted: 1.0 on exp_avg_sq.

The key biases are why: a key bias adds the same number to every score of a query, softmax does not see it, so its gradient is
zero in exact arithmetic and what the kernels compute for it is rounding noise of the order-dependent sums; Adam divides that
noise by its own root mean square and moves the bias by about lr per step in a direction no two runs share.  These tensors
(NOISE_ONLY: the model's four key biases, named one by one) carry no information about the trajectory and are left out of
the numeric comparison -- the uninterrupted run does not reproduce them against ITSELF; test A compares them exactly like every other tensor.  For the rest the
spread, 3.6e-5 at its worst, is more than a tenth of the project's fp32 bar (tests/util.TOL, 1e-4), so the bar is ten times the spread: 3.6e-4,
of which BAR = 3e-4 stays a little inside.  The
negative control of B -- the second half from the weights alone, with a fresh optimizer -- must miss BAR on exp_avg_sq by 100x,
or these tests could not see the moments at all."""
import functools
import os
import random
import re
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

from tests.util import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(lang_dec=False, enc_layer=2, dec_layer=2, embed_dim=128, intermediate_dim=512, num_attention_heads=4)
SEED = 21
BAR = 3e-4  # just inside 10 x the measured run-to-run spread (above); tests/util.TOL[float32] = 1e-4 is less than 10 x that spread
# tensors whose gradient is zero in exact arithmetic (above): not compared between two runs.  At toy size these are FOUR: the key
# biases of the two encoder self-attentions and of the two cross-attentions.  There is no other ``key.bias`` in this model: with
# as many decoder layers as encoder layers the decoder's self-attention IS the encoder's module (seq2seq.py), under the
# encoder's name.  They are named one by one, so that nothing else can fall under the exclusion.
NOISE_ONLY = ("encoder.encoder.layer.0.attention.self.key.bias", "encoder.encoder.layer.1.attention.self.key.bias",
              "decoder.decoder.layer.0.crossattention.self.key.bias", "decoder.decoder.layer.1.crossattention.self.key.bias")
SEEDS = []  # every seed handed to mass_mask_device, in call order (record_seeds)


# ------------------------------------------------------------------------------------------------ the toy run
@functools.lru_cache(maxsize=None)
def toy_data():
    """(MT batches, MASS batches) of a few dozen short sentences over 300 ids: 4-8 batches per kind."""
    from imagetranslate_amd.dataset import MassDataset, MTDataset
    rnd = random.Random(3)
    sents = sorted(([rnd.randint(7, 299) for _ in range(rnd.randint(6, 18))] for _ in range(40)), key=len)
    pairs = [([5] + s + [4], [6] + [299 + 7 - w for w in reversed(s)] + [4], 0, 1) for s in sents]
    mt = MTDataset(max_batch_capacity=50, max_batch=320, pad_idx=0, max_seq_len=64, examples=pairs)
    mono = [[5] + [rnd.randint(7, 299) for _ in range(rnd.randint(8, 20))] + [4] for _ in range(44)]
    mono.sort(key=len)
    mass = MassDataset(None, max_batch_capacity=50, max_batch=320, pad_idx=0, max_seq_len=64, example_list=[[(s, 0) for s in mono]])
    assert 4 <= len(mt) <= 8 and 4 <= len(mass) <= 8, (len(mt), len(mass))
    return mt, mass


def make(seed, dtype=torch.float32, rank=0, world=1):
    """A fresh toy model, optimizer (lr 2e-3, warm-up 4: large updates, a missing moment shows) and trainer; torch's and
    Python's generators are seeded with ``seed``, like the trainers' ``train()``."""
    from imagetranslate_amd.image_model import ImageMassSeq2Seq
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    from imagetranslate_amd.train_image_mt import ImageMTTrainer
    from imagetranslate_amd.utils import build_optimizer
    random.seed(seed)
    torch.manual_seed(seed)
    model = ImageMassSeq2Seq(SyntheticTextProcessor(300), **KW)
    model.set_compute_dtype(dtype)
    model = model.cuda().train()
    return ImageMTTrainer(model, mask_prob=0.3, optimizer=build_optimizer(model, 2e-3, 4), rank=rank, world_size=world, seed=seed)


def record(trainer):
    """Wrap the trainer's step methods: log["visited"] gets the (kind, index) of every batch stepped on, log["lr"] the learning
    rate after it."""
    mt, mass = toy_data()
    names = {id(b): ("mt", i) for i, b in enumerate(mt.batches)}
    names.update({id(b): ("mass", i) for i, b in enumerate(mass.batches)})
    log = {"visited": [], "lr": []}

    def wrap(fn):
        def step(batch, *a, **kw):
            out = fn(batch, *a, **kw)
            log["visited"].append(names[id(batch)])
            log["lr"].append(trainer.optimizer.param_groups[0]["lr"])
            return out
        return step

    trainer.mt_step, trainer.mass_step = wrap(trainer.mt_step), wrap(trainer.mass_step)
    return log


def run(trainer, steps, accum=1):
    """The epoch loop over the toy data until ``steps`` counted steps in all."""
    mt, mass = toy_data()
    step = trainer.step
    while step < steps:
        step = trainer.train_epoch(mt_data=mt, mass_data=mass, step=step, max_step=steps, log_every=10 ** 6, accum=accum)
    torch.cuda.synchronize()
    return step


def buffers(trainer):
    """{"weights" | "exp_avg" | "exp_avg_sq": {state-dict key: CPU tensor}} of the trainer's flat store."""
    from imagetranslate_amd.checkpoint import store_layout
    st, layout = store_layout(trainer.model)
    st.wait_updates(0)
    m, v = st.moments()
    torch.cuda.synchronize()
    return {name: {k: st._view(buf, p).detach().cpu().clone() for k, p in layout}
            for name, buf in (("weights", st.flat), ("exp_avg", m), ("exp_avg_sq", v))}


def distance(got, want, skip=NOISE_ONLY):
    """Worst per-tensor rel_err of ``got`` against ``want`` (both from ``buffers``), per buffer, over the tensors not named in
    ``skip``."""
    skip = tuple(skip or ())
    assert all(k in want["weights"] for k in skip), "a tensor to leave out is not there"
    keys = [k for k in want["weights"] if k not in skip]
    return {name: max(rel_err(got[name][k], want[name][k]) for k in keys) for name in want}


def fresh_optimizer(trainer):
    """What a restart from the weights alone has: zero moments, no updates, the schedule at its start."""
    opt = trainer.optimizer
    n = sum(len(g["params"]) for g in opt.param_groups)
    opt.load_state_dict({"state": {}, "param_groups": [{"num_updates": 0, "params": list(range(n))}]})


@pytest.fixture
def record_seeds(monkeypatch):
    from imagetranslate_amd import train_image_mt
    real = train_image_mt.mass_mask_device

    def spy(*a, seed, **kw):
        SEEDS.append(seed)
        return real(*a, seed=seed, **kw)

    monkeypatch.setattr(train_image_mt, "mass_mask_device", spy)
    del SEEDS[:]
    return SEEDS


def continuation(tmp_path, first, total, accum=1):
    """The uninterrupted run of ``total`` steps, the run stopped after ``first`` steps + snapshot + fresh objects (another seed)
    + load + the rest, and the control (the same, but with a fresh optimizer after the load).  Returns what the tests and
    tools/resume_measure.py compare."""
    from imagetranslate_amd.checkpoint import load_train_state, save_train_state
    path = str(tmp_path / "train_state.pt")
    out = {}
    whole = make(SEED)
    log = record(whole)
    del SEEDS[:]
    run(whole, total, accum)
    out["whole"] = dict(log, seeds=list(SEEDS), rng=torch.get_rng_state(), buffers=buffers(whole), trainer=whole)
    head = make(SEED)
    hlog = record(head)
    del SEEDS[:]
    run(head, first, accum)
    save_train_state(path, head)
    tail = make(SEED + 1)
    load_train_state(path, tail)
    tlog = record(tail)
    run(tail, total, accum)
    out["resumed"] = dict(visited=hlog["visited"] + tlog["visited"], lr=hlog["lr"] + tlog["lr"], seeds=list(SEEDS),
                          rng=torch.get_rng_state(), buffers=buffers(tail), trainer=tail)
    ctrl = make(SEED + 1)
    load_train_state(path, ctrl)
    fresh_optimizer(ctrl)
    run(ctrl, total, accum)
    out["control"] = dict(buffers=buffers(ctrl))
    return out


def assert_continues(out, total_updates):
    whole, resumed = out["whole"], out["resumed"]
    assert resumed["visited"] == whole["visited"] and {k for k, _ in whole["visited"]} == {"mt", "mass"}
    assert resumed["seeds"] == whole["seeds"] and len(whole["seeds"]) == sum(k == "mass" for k, _ in whole["visited"])
    assert torch.equal(resumed["rng"], whole["rng"])
    assert resumed["lr"] == whole["lr"]
    for t in (whole["trainer"], resumed["trainer"]):
        assert t.optimizer.param_groups[0]["num_updates"] == total_updates
    dist = distance(resumed["buffers"], whole["buffers"])
    print("resumed vs uninterrupted:", dist)
    assert max(dist.values()) <= BAR, dist
    return dist


# ------------------------------------------------------------------------------------------------ A. exact round trip
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_snapshot_round_trip_is_exact(cuda, tmp_path, dtype):
    from imagetranslate_amd.checkpoint import load_train_state, save_train_state, store_layout
    mt, mass = toy_data()
    a = make(SEED, dtype)
    for k in range(5):  # alternating MT and MASS batches
        if k % 2 == 0:
            a.mt_step(mt[k // 2])
        else:
            a.mass_step(mass[k // 2])
    a.step, a.epoch, a.epoch_pos, a.best_loss = 5, 1, 5, 1.5
    path = str(tmp_path / "train_state.pt")
    save_train_state(path, a)
    assert not os.path.exists(path + ".tmp")
    torch.load(path, weights_only=True)
    b = make(SEED + 7, dtype)
    st_b, layout_b = store_layout(b.model)
    if dtype == torch.bfloat16:
        st_b.params_for(torch.bfloat16)  # a bf16 shadow of the OLD weights exists: the load must not leave it standing
    load_train_state(path, b)
    st_a, layout_a = store_layout(a.model)
    st_a.wait_updates(0)
    assert [k for k, _ in layout_a] == [k for k, _ in layout_b]
    for buf_a, buf_b in zip((st_a.flat,) + st_a.moments(), (st_b.flat,) + st_b.moments()):
        for (k, p), (_, q) in zip(layout_a, layout_b):
            assert torch.equal(st_a._view(buf_a, p), st_b._view(buf_b, q)), k
    assert float(st_a.exp_avg_sq.abs().max()) > 0
    ga, gb = a.optimizer.param_groups[0], b.optimizer.param_groups[0]
    assert (gb["num_updates"], gb["lr"]) == (ga["num_updates"], ga["lr"]) == (5, a.optimizer.get_lr_for_step(5))
    assert (b.step, b.epoch, b.epoch_pos, b.micro_step, b.best_loss) == (5, 1, 5, 5, 1.5)
    assert b.seed == a.seed == SEED
    if dtype == torch.bfloat16:
        assert torch.equal(st_b.params_for(torch.bfloat16), st_b.flat.to(torch.bfloat16))
    # the next 10 draws of every restored generator: the original's (drawn AFTER the snapshot, from the same state)
    expect = ([random.random() for _ in range(10)], torch.rand(10), [a._mass_rng.getrandbits(62) for _ in range(10)],
              [a._img_rng.random() for _ in range(10)])
    random.seed(0)
    torch.manual_seed(0)
    load_train_state(path, b)
    assert [random.random() for _ in range(10)] == expect[0] and torch.equal(torch.rand(10), expect[1])
    assert [b._mass_rng.getrandbits(62) for _ in range(10)] == expect[2] and [b._img_rng.random() for _ in range(10)] == expect[3]


def test_optimizer_state_dict_holds_the_fused_moments(cuda):
    mt, _ = toy_data()
    a = make(SEED)
    a.mt_step(mt[0])
    sd = a.optimizer.state_dict()
    params = list(a.model.parameters())
    assert len(sd["state"]) == len(params) and sd["param_groups"][0]["num_updates"] == 1
    assert all(sd["state"][i]["exp_avg_sq"].shape == p.shape for i, p in enumerate(params))
    assert max(float(s["exp_avg_sq"].max()) for s in sd["state"].values()) > 0


# ------------------------------------------------------------------------------------------------ B. continuation
def test_resumed_run_continues_the_uninterrupted_run(cuda, tmp_path, record_seeds):
    out = continuation(tmp_path, 6, 12)
    assert_continues(out, 12)
    control = distance(out["control"]["buffers"], out["whole"]["buffers"])
    print("weights-only control vs uninterrupted:", control)
    assert control["exp_avg_sq"] >= 100 * BAR, "the test cannot see a missing second moment: %r" % (control,)


# ------------------------------------------------------------------------------------------------ C. accumulation
def test_snapshot_waits_for_the_accumulation_window_and_the_run_continues(cuda, tmp_path, record_seeds):
    from imagetranslate_amd.checkpoint import load_train_state
    directory = str(tmp_path / "m.latest")
    path = os.path.join(directory, "train_state.pt")
    whole = make(SEED)
    wlog = record(whole)
    run(whole, 8, accum=2)
    seeds_whole, rng_whole = list(SEEDS), torch.get_rng_state()
    head = make(SEED)
    hlog = record(head)
    del SEEDS[:]
    head.enable_snapshots(directory, save_steps=3, accum=2)
    seen = []  # (micro-steps done, is the file there) when each step begins

    def watch(fn):
        def step(batch, *a, **kw):
            seen.append((head.micro_step, os.path.exists(path)))
            return fn(batch, *a, **kw)
        return step

    head.mt_step, head.mass_step = watch(head.mt_step), watch(head.mass_step)
    run(head, 4, accum=2)
    assert seen == [(0, False), (1, False), (2, False), (3, False)], "due after step 3, an odd micro-step: no file yet"
    assert os.path.exists(path) and torch.load(path, weights_only=True)["trainer"]["micro_step"] == 4
    assert os.path.exists(os.path.join(directory, "mt_model.state_dict")), "the model's own save() output is there too"
    tail = make(SEED + 1)
    load_train_state(path, tail)
    tlog = record(tail)
    run(tail, 8, accum=2)
    out = {"whole": dict(wlog, seeds=seeds_whole, rng=rng_whole, buffers=buffers(whole), trainer=whole),
           "resumed": dict(visited=hlog["visited"] + tlog["visited"], lr=hlog["lr"] + tlog["lr"], seeds=list(SEEDS),
                           rng=torch.get_rng_state(), buffers=buffers(tail), trainer=tail)}
    assert_continues(out, 4)
    assert tail.micro_step == whole.micro_step == 8


# ------------------------------------------------------------------------------------------------ D, E. command line
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Tokenizer, sentence-pair batches and monolingual batches of a 200-sentence synthetic corpus."""
    from imagetranslate_amd import create_mt_batches, train_tokenizer
    from tests.test_gpu_cli import _corpus
    d = str(tmp_path_factory.mktemp("resume_cli"))
    src, dst = _corpus(200, 5)
    with open(os.path.join(d, "all.txt"), "w") as fw:
        fw.write("\n".join(["<xa> " + s + " </s>" for s in src] + ["<xb> " + t + " </s>" for t in dst]) + "\n")
    for name, lines in (("train.xa", src), ("train.xb", dst)):
        with open(os.path.join(d, name), "w") as fw:
            fw.write("\n".join(lines) + "\n")
    tok = os.path.join(d, "tok")
    train_tokenizer.main(["--data", os.path.join(d, "all.txt"), "--vocab_size", "400", "--model", tok])
    create_mt_batches.main(["--src", os.path.join(d, "train.xa"), "--dst", os.path.join(d, "train.xb"), "--src-lang", "xa",
                            "--dst-lang", "xb", "--tok", tok, "--output", os.path.join(d, "train.batch")])
    create_mt_batches.main(["--src", os.path.join(d, "train.xa"), "--src-lang", "xa", "--tok", tok, "--output", os.path.join(d, "mono.xa")])
    return {"dir": d, "tok": tok, "mt": os.path.join(d, "train.batch"), "mono": os.path.join(d, "mono.xa")}


def cli(files, model_dir, *more):
    from imagetranslate_amd import train_image_mt
    args = ["--tok", files["tok"], "--model", model_dir, "--embed", "128", "--intermediate", "512", "--enc", "2", "--dec", "2",
            "--heads", "4", "--batch", "1500", "--capacity", "50", "--lr", "0.002", "--warmup", "4", "--epoch", "40",
            "--log-steps", "1", "--fp32"] + list(more)
    opts, _ = train_image_mt.get_option_parser().parse_args(args)
    return train_image_mt.train(opts)


def logged_steps(out):
    return [int(m.group(1)) for m in re.finditer(r" step (\d+) loss ", out)]


def test_command_line_saves_state_and_resumes(cuda, files, tmp_path, capsys):
    from imagetranslate_amd.image_model import ImageMassSeq2Seq
    model_dir = str(tmp_path / "model")
    latest = model_dir + ".latest"
    first = cli(files, model_dir, "--train_mt", files["mt"], "--save-state", "--save-steps", "4", "--step", "8")
    assert logged_steps(capsys.readouterr().out) == list(range(1, 9))
    assert first.optimizer.param_groups[0]["num_updates"] == 8
    blob = torch.load(os.path.join(latest, "train_state.pt"), weights_only=True)
    assert blob["trainer"]["step"] == 8 and blob["num_updates"] == 8 and blob["trainer"]["phase"] == "train"
    assert {"mt_config", "mt_model.state_dict", "train_state.pt"} <= set(os.listdir(latest))
    assert not [f for f in os.listdir(latest) if f.endswith(".tmp")]
    second = cli(files, model_dir, "--train_mt", files["mt"], "--resume", latest, "--step", "12")
    steps = logged_steps(capsys.readouterr().out)
    assert steps == [9, 10, 11, 12], "the resumed run logs no step <= 8"
    assert second.optimizer.param_groups[0]["num_updates"] == 12 and second.step == 12
    assert second.optimizer.param_groups[0]["lr"] == second.optimizer.get_lr_for_step(12)
    model = ImageMassSeq2Seq.load(ImageMassSeq2Seq, latest, tok_dir=files["tok"])  # what --pretrained <model>.latest does
    assert model.config.num_attention_heads == 4


def test_resume_inside_the_back_translation_phase(cuda, files, tmp_path, capsys):
    model_dir = str(tmp_path / "model")
    latest = model_dir + ".latest"
    common = ["--mass_train", files["mono"], "--langs", "xa,xb", "--step", "2", "--bt-sampling", "--save-state", "--save-steps", "3"]
    first = cli(files, model_dir, *common, "--fstep", "2")
    assert first.phase == "bt" and first.step == 4 and first.generator.searches == 2
    assert first.optimizer.param_groups[0]["num_updates"] == 2, "the schedule was reset when the phase began"
    blob = torch.load(os.path.join(latest, "train_state.pt"), weights_only=True)
    assert blob["trainer"]["phase"] == "bt" and blob["trainer"]["step"] == 4 and blob["trainer"]["phase_start_step"] == 2
    assert blob["ranks"][0]["searches"] == 2 and blob["num_updates"] == 2
    capsys.readouterr()
    second = cli(files, model_dir, *common, "--fstep", "4", "--resume", latest)
    assert logged_steps(capsys.readouterr().out) == [5, 6]
    assert second.phase == "bt" and second.step == 6
    assert second.generator.searches == 4, "the sampled searches continue the saved count once the generator is built"
    assert second.optimizer.param_groups[0]["num_updates"] == 4, "no second reset()"


# ------------------------------------------------------------------------------------------------ F. two ranks on one GPU
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_run(rank, world, port, out_dir, mode, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from imagetranslate_amd import train_image_mt
        from imagetranslate_amd.checkpoint import load_train_state, save_train_state
        torch.cuda.set_device(0)
        real = train_image_mt.mass_mask_device

        def spy(*a, seed, **kw):
            SEEDS.append(seed)
            return real(*a, seed=seed, **kw)

        train_image_mt.mass_mask_device = spy
        path = os.path.join(out_dir, "train_state.pt")

        def report(tag, trainer, log):
            torch.save({"buffers": buffers(trainer), "visited": log["visited"], "seeds": list(SEEDS),
                        "next_mass_draw": trainer._mass_rng.getrandbits(62), "step": trainer.step},
                       os.path.join(out_dir, "%s_rank%d.pt" % (tag, rank)))

        if mode == "first":
            whole = make(SEED, rank=rank, world=world)
            log = record(whole)
            run(whole, 6)
            report("whole", whole, log)
            del SEEDS[:]
            head = make(SEED, rank=rank, world=world)
            run(head, 4)
            save_train_state(path, head)  # every rank: the streams are gathered, rank 0 writes
        else:
            tail = make(SEED + 1, rank=rank, world=world)
            load_train_state(path, tail)
            log = record(tail)
            run(tail, 6)
            report("resumed", tail, log)
        dist.barrier()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: %s\n%s" % (e, traceback.format_exc())))
    finally:
        dist.destroy_process_group()


def _two_ranks(out_dir, mode):
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank_run, args=(r, 2, port, out_dir, mode, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(30)
    assert all(r[1] == "ok" for r in res), [r[1] for r in res]


@pytest.mark.timeout(600)
def test_two_ranks_resume_their_own_streams(cuda, tmp_path):
    from imagetranslate_amd.checkpoint import load_train_state
    out_dir = str(tmp_path)
    _two_ranks(out_dir, "first")
    blob = torch.load(os.path.join(out_dir, "train_state.pt"), weights_only=True)
    assert blob["trainer"]["world_size"] == 2 and len(blob["ranks"]) == 2 and blob["trainer"]["step"] == 4
    assert blob["ranks"][0]["mass_rng"] != blob["ranks"][1]["mass_rng"]
    _two_ranks(out_dir, "resume")
    load = lambda tag, r: torch.load(os.path.join(out_dir, "%s_rank%d.pt" % (tag, r)), weights_only=True)
    whole, resumed = [load("whole", r) for r in (0, 1)], [load("resumed", r) for r in (0, 1)]
    assert any(k == "mass" for r in (0, 1) for k, _ in whole[r]["visited"][:4]), "the first four steps include MASS batches"
    for r in (0, 1):
        assert resumed[r]["step"] == 6 and resumed[r]["visited"] == whole[r]["visited"][4:]
        n = len(resumed[r]["seeds"])
        assert resumed[r]["seeds"] == whole[r]["seeds"][len(whole[r]["seeds"]) - n:]
        assert resumed[r]["next_mass_draw"] == whole[r]["next_mass_draw"], "rank %d continues its own stream" % r
    assert resumed[0]["next_mass_draw"] != resumed[1]["next_mass_draw"]
    for name in ("weights", "exp_avg", "exp_avg_sq"):
        for k, v in resumed[0]["buffers"][name].items():
            assert torch.equal(v, resumed[1]["buffers"][name][k]), "the ranks diverged on %s %s" % (name, k)
    dist = distance(resumed[0]["buffers"], whole[0]["buffers"])
    print("two ranks, resumed vs uninterrupted:", dist)
    assert max(dist.values()) <= BAR, dist
    with pytest.raises(ValueError, match="world_size 2.*world_size 1"):
        load_train_state(os.path.join(out_dir, "train_state.pt"), make(SEED))


# ------------------------------------------------------------------------------------------------ another entry point
def test_train_txt_sim_saves_state_and_resumes(cuda, tmp_path, capsys, monkeypatch):
    """The base-class hooks through an entry point other than train_image_mt: train_txt_sim builds its model from the flags,
    writes train_state.pt into its own ``.latest`` write, and the resumed run draws the negatives of the steps it runs."""
    from imagetranslate_amd import train_txt_sim as S
    from tests.test_gpu_sensim import _files
    tok, tp, n_dev = _files(tmp_path)
    d = str(tmp_path)
    draws = []
    real = S.draw_negative
    monkeypatch.setattr(S, "draw_negative", lambda seed, step, side, n: draws.append((step, side)) or real(seed, step, side, n))

    def train(out, *more):
        argv = ["--tok", tok, "--train_mt", os.path.join(d, "train.mt"), "--src-neg", os.path.join(d, "neg.src"), "--dst-neg",
                os.path.join(d, "neg.dst"), "--model", out, "--enc", "1", "--embed", "128", "--intermediate", "256", "--heads", "4",
                "--lr", "0.001", "--warmup", "5", "--batch", "1200", "--capacity", "50", "--max_seq_len", "80", "--fp32", "--seed", "7",
                "--log-steps", "1", "--save-steps", "3", "--save-state"] + list(more)
        del draws[:]
        trainer = S.SenSimTrainer.train(S.add_resume_options(S.get_img_options_parser()).parse_args(argv)[0])
        steps = [int(m.group(1)) for m in re.finditer(r"Epoch Step: (\d+) ", capsys.readouterr().out)]
        return trainer, steps, list(draws)

    whole, steps, whole_draws = train(os.path.join(d, "whole"), "--step", "9")
    assert steps == list(range(1, 10)) and whole_draws == [(s, side) for s in range(9) for side in (0, 1)]
    out = os.path.join(d, "sim")
    first, steps, _ = train(out, "--step", "6")
    assert steps == list(range(1, 7))
    assert sorted(os.listdir(out + ".latest")) == ["imt_config.json", "mt_config", "mt_model.state_dict", "train_state.pt"]
    blob = torch.load(os.path.join(out + ".latest", "train_state.pt"), weights_only=True)
    assert blob["model_class"] == "SenSim" and blob["trainer"]["step"] == 6 and blob["num_updates"] == 6
    second, steps, second_draws = train(out, "--step", "9", "--resume", out + ".latest")
    assert steps == [7, 8, 9] and second_draws == whole_draws[12:]
    assert second.optimizer.param_groups[0]["num_updates"] == 9 and (second.step, second.epoch) == (whole.step, whole.epoch)
    assert second.optimizer.param_groups[0]["lr"] == whole.optimizer.param_groups[0]["lr"]
    # (the trajectory itself is compared in B, C and F on the model whose run-to-run spread was measured)
