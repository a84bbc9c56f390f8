"""Snapshots of a training run (``--save-state`` / ``--resume``): ONE file, ``train_state.pt``, that holds what ``model.save()``
does not -- the Adam moments, the update count that drives the learning-rate schedule, the position in the epoch and every
random stream -- plus the fp32 master weights, so that the file is complete on its own.

The file is a dict of tensors, ints, floats, strings, lists, tuples and None only: ``torch.load(weights_only=True)`` reads it,
like ``mt_model.state_dict`` and ``features.pt``; no optimizer or generator OBJECT is pickled (the reference's --save-opt file is a
pickled optimizer, which this package never unpickles: safe_pickle.py).  It is written to ``train_state.pt.tmp`` beside its
place and moved there with ``os.replace``: a writer that dies midway leaves the previous ``train_state.pt`` as it was (this file
only: the model's own ``save()`` files beside it are overwritten in place).

Tensors are keyed by the reference's state-dict names (``weights/<key>``, ``exp_avg/<key>``, ``exp_avg_sq/<key>``), one entry per
parameter of the flat store under the first name the model gives it (a tied parameter is stored once), so a snapshot survives a
change of the flat layout.  Under data parallelism rank 0 writes; the ranks' random streams are gathered into ``ranks`` and every
rank takes its own entry back.  Parameters and moments are rank 0's: the replicas are bit-identical by construction."""
import os

import torch

from .param_store import store_of

FORMAT_VERSION = 1
STATE_FILE = "train_state.pt"


def store_layout(model):
    """(store, [(state-dict key, parameter)]) for every entry of the model's flat store, in store order."""
    st = store_of(model).ensure()
    names = {}
    for name, p in model.named_parameters():  # (duplicates removed: a tied parameter appears under its first name)
        names.setdefault(id(p), name)
    return st, [(names[id(p)], p) for p, _, _ in st.entries]


def _world():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 else None


def save_train_state(path: str, trainer, **progress):
    """Write the snapshot of ``trainer`` (its model, optimizer and own state) to ``path``; ``progress``: further plain values
    that ``load_train_state`` hands back.  Under data parallelism EVERY rank calls this (the ranks' streams are gathered)."""
    model, optimizer = trainer.model, trainer.optimizer
    state = trainer.state_dict()
    mine = state.pop("rank")
    ranks, dist = [mine], _world()
    if dist is not None:
        ranks = [None] * dist.get_world_size()
        dist.all_gather_object(ranks, mine)
    if len(ranks) != int(trainer.world_size):
        raise ValueError("the trainer has world_size %d but %d rank(s) took part in the snapshot" % (trainer.world_size, len(ranks)))
    if trainer.rank != 0:
        return
    st, layout = store_layout(model)
    st.wait_updates(0)
    fused = optimizer._store() is st  # the moments live in the store: each span goes straight to the host, no device copy
    opt = {"state": {}} if fused else optimizer.state_dict()
    opt_index = {id(p): i for i, p in enumerate(p for g in optimizer.param_groups for p in g["params"])}
    blob = {"format_version": FORMAT_VERSION, "model_class": type(model).__name__,
            "layout": [(key, [int(d) for d in p.shape]) for key, p in layout],
            "num_updates": int(optimizer.param_groups[0]["num_updates"]), "trainer": state, "ranks": ranks,
            "progress": dict(progress)}
    for key, p in layout:
        blob["weights/" + key] = st._view(st.flat, p).detach().to("cpu", copy=True)
        moments = opt["state"].get(opt_index.get(id(p)))
        if fused and st.exp_avg is not None and id(p) in opt_index:
            moments = {"exp_avg": st._view(st.exp_avg, p), "exp_avg_sq": st._view(st.exp_avg_sq, p)}
        for k in ("exp_avg", "exp_avg_sq"):
            blob[k + "/" + key] = torch.zeros(p.shape) if moments is None else moments[k].detach().float().to("cpu", copy=True)
    tmp = path + ".tmp"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    try:
        torch.save(blob, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def load_train_state(path: str, trainer) -> dict:
    """Put the snapshot at ``path`` back: master weights (the bf16 shadow is rebuilt before the next forward), moments and
    update count, the trainer's counters and THIS rank's random streams.  Returns the trainer's part of the file with the
    ``progress`` values of ``save_train_state`` merged in.  Refuses, naming what differs: an unknown format version, another
    model class, a layout that differs in a key or a shape (the first mismatch), another world size."""
    blob = torch.load(path, map_location="cpu", weights_only=True)
    if blob.get("format_version") != FORMAT_VERSION:
        raise ValueError("%s: format_version %r, this build reads %d" % (path, blob.get("format_version"), FORMAT_VERSION))
    model, optimizer = trainer.model, trainer.optimizer
    if blob["model_class"] != type(model).__name__:
        raise ValueError("%s: snapshot of a %s model, this trainer has a %s" % (path, blob["model_class"], type(model).__name__))
    st, layout = store_layout(model)
    saved = [(k, tuple(int(d) for d in shape)) for k, shape in blob["layout"]]
    # the entries are matched by key, not by place: the order of the flat store may have changed since the snapshot
    ours = {k: tuple(p.shape) for k, p in layout}
    for k, shape in saved:
        if k not in ours:
            raise ValueError("%s: layout entry %s %s of the snapshot is no parameter of this model" % (path, k, shape))
        if ours[k] != shape:
            raise ValueError("%s: layout entry %s is %s in the snapshot, %s in this model" % (path, k, shape, ours[k]))
    saved_keys = {k for k, _ in saved}
    for k, p in layout:
        if k not in saved_keys:
            raise ValueError("%s: parameter %s %s of this model is no layout entry of the snapshot" % (path, k, tuple(p.shape)))
    tstate = dict(blob["trainer"])
    if int(tstate["world_size"]) != int(trainer.world_size) or len(blob["ranks"]) != int(trainer.world_size):
        raise ValueError("%s: the snapshot was taken with world_size %d, this run has world_size %d (resuming at another "
                         "world size is not built)" % (path, int(tstate["world_size"]), int(trainer.world_size)))
    # weights: into the fp32 master through the flat buffer; mark_master_changed() makes the next bf16 consumer recast it
    st.wait_updates(0)
    with torch.no_grad():
        for key, p in layout:
            st._view(st.flat, p).copy_(blob["weights/" + key])
    st.mark_master_changed()
    # moments and update count: in the optimizer's own parameter order
    index = {id(p): key for key, p in layout}
    params = [p for g in optimizer.param_groups for p in g["params"]]
    opt_state = {i: {k: blob[k + "/" + index[id(p)]] for k in ("exp_avg", "exp_avg_sq")} for i, p in enumerate(params)}
    groups, n = [], 0
    for g in optimizer.param_groups:
        groups.append({"num_updates": int(blob["num_updates"]), "params": list(range(n, n + len(g["params"])))})
        n += len(g["params"])
    optimizer.load_state_dict({"state": opt_state, "param_groups": groups})
    tstate["rank"] = blob["ranks"][int(trainer.rank)]
    trainer.load_state_dict(tstate)
    out = {k: v for k, v in tstate.items() if k != "rank"}
    out.update(blob.get("progress", {}))
    return out
