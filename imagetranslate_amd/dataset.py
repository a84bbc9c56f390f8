"""On-disk example files and batch construction -- drop-in for the text parts of the reference's ``src/dataset.py``
(``MTDataset`` ``:73-168``, ``MassDataset`` ``:171-270``) and the example files written by
``src/create_mt_batches.py:8-71``.

File format (unchanged, so files written by the reference load here and vice versa): a ``marshal`` dump of a list of
``(src_ids, dst_ids, src_lang, dst_lang)`` tuples sorted by target length (parallel data), or of
``(src_ids, lang)`` tuples sorted by length (monolingual data for MASS, possibly split into ``<path>.<part>`` files).

Batches are whole pre-padded tensors (the trainer's DataLoader uses ``batch_size=1``): sentences are taken in file
order and a batch is closed as soon as adding the next sentence would exceed either budget
    parallel : (S + T) * n > max_batch          or  (S^2 + T^2) * n * T > max_batch_capacity * 1e6
    MASS     : 2 * S * n   > max_batch          or  2 * S^3 * n         > max_batch_capacity * 1e6
(S, T = longest source / target in the batch including the candidate, n = sentences including the candidate), as
long as the batch without the candidate keeps at least ``ngpu`` sentences.  The shapes this produces (length-sorted,
ragged) are what the kernels see in real training.
"""
import glob
import marshal
import os
import random
from typing import List, Optional

import torch
from torch.nn.utils.rnn import pad_sequence
from torch.utils.data import Dataset


def _first_pad_index(texts: torch.Tensor, pad_idx: int) -> torch.Tensor:
    """Per row: index of the first pad token, or width-1 when the row has none (reference ``pad_idx_find``)."""
    is_pad = texts == pad_idx
    width = texts.size(1)
    first = torch.where(is_pad.any(dim=1), is_pad.to(torch.int8).argmax(dim=1), torch.full((texts.size(0),), width - 1))
    return first.to(torch.long)


def get_lex_dict(path: str) -> dict:
    """The --dict file (src/train_image_mt.py:29-36): lines of ``id id id ...``; the first id is the key, the others its
    proposed translations (lines with the same key add up)."""
    lex_dict = {}
    with open(path) as fp:
        for line in fp:
            ids = [int(x) for x in line.split()]
            if ids:
                lex_dict.setdefault(ids[0], []).extend(ids[1:])
    return lex_dict


def get_lex_suggestions(lex_dict, ids, pad_idx: int) -> torch.Tensor:
    """Proposed word ids of one sentence (src/dataset.py:23-27): the union of ``lex_dict[int(w)]`` over its tokens, sorted
    (the reference's order is a set's; the proposal attention does not depend on it), or ``[pad_idx]`` when no token has an
    entry.  Keys are looked up as ints whether ``ids`` is a tensor or a list -- the reference looks up 0-d tensors, which hash
    by identity and never hit."""
    found = set()
    for w in (ids.tolist() if torch.is_tensor(ids) else ids):
        found.update(lex_dict.get(int(w), ()))
    return torch.LongTensor(sorted(found)) if found else torch.LongTensor([pad_idx])


def _pad_proposals(lex: List[torch.Tensor], pad_idx: int) -> torch.Tensor:
    return pad_sequence(lex, batch_first=True, padding_value=pad_idx)


class TextDataset(Dataset):
    """Rows of the marshal blocks ``create_batches.write`` leaves in ``save_cache_dir`` (src/dataset.py:30-70): item ``i`` is
    ``(ids, language index)`` from block ``i // block size``.  At most ``max_cache_size`` blocks are held: a row of a block that
    is not held replaces the cache by that block and the ones after it.  ``load_all`` reads every block up front."""

    def __init__(self, save_cache_dir: str, max_cache_size: int = 100, load_all: bool = False):
        self.current_cache = {}
        self.max_cache_size = max_cache_size
        self.save_cache_dir = save_cache_dir
        with open(os.path.join(save_cache_dir, "info.txt"), "r") as fr:
            block, lines, files = fr.read().strip().split("\t")
        self.sentence_block_size, self.line_num, self.file_count = int(block), int(lines), int(files)
        if load_all:
            self.rebuild_cache(0, self.file_count)

    def __len__(self):
        return self.line_num

    def rebuild_cache(self, start_file_num: int, end_file_num: int):
        self.current_cache = {}
        for file_num in range(start_file_num, end_file_num):
            with open(os.path.join(self.save_cache_dir, str(file_num) + ".pkl"), "rb") as fp:
                self.current_cache[file_num] = marshal.load(fp)

    def __getitem__(self, item):
        if not 0 <= item < self.line_num:
            raise IndexError(item)
        file_num = item // self.sentence_block_size
        if file_num not in self.current_cache:
            self.rebuild_cache(file_num, min(self.file_count, file_num + self.max_cache_size))
        return self.current_cache[file_num][item]


class TextCollator:
    """Rows of ``TextDataset`` -> {"texts" [B, S], "pad_mask" (True on real tokens), "langs" [B]} (src/dataset.py:479-490)."""

    def __init__(self, pad_idx: int):
        self.pad_idx = pad_idx

    def __call__(self, batch):
        texts = pad_sequence([torch.LongTensor(ids) for ids, _ in batch], batch_first=True, padding_value=self.pad_idx)
        return {"texts": texts, "pad_mask": texts != self.pad_idx, "langs": torch.LongTensor([lang for _, lang in batch])}


class MTDataset(Dataset):
    def __init__(self, max_batch_capacity: int, max_batch: int, pad_idx: int, max_seq_len: int = 175,
                 batch_pickle_dir: Optional[str] = None, examples: Optional[List] = None, lex_dict=None,
                 keep_pad_idx: bool = True, ngpu: int = 1):
        self.lex_dict = lex_dict
        self.keep_pad_idx = keep_pad_idx
        self.ngpu = ngpu
        if examples is None:
            with open(batch_pickle_dir, "rb") as fr:
                examples = marshal.load(fr)
        self.batch_examples(examples, max_batch, max_batch_capacity, max_seq_len, ngpu, pad_idx)

    def _emit(self, src, dst, src_langs, dst_langs, pad_idx, lex=None):
        src_batch = pad_sequence(src, batch_first=True, padding_value=pad_idx)
        dst_batch = pad_sequence(dst, batch_first=True, padding_value=pad_idx)
        entry = {"src_texts": src_batch, "src_pad_mask": src_batch != pad_idx, "dst_texts": dst_batch,
                 "dst_pad_mask": dst_batch != pad_idx, "src_langs": torch.LongTensor(src_langs),
                 "dst_langs": torch.LongTensor(dst_langs),
                 "proposal": _pad_proposals(lex, pad_idx) if self.lex_dict is not None else torch.LongTensor([pad_idx])}
        if self.keep_pad_idx:
            entry["pad_idx"] = _first_pad_index(src_batch, pad_idx)
        self.batches.append(entry)

    def batch_examples(self, examples, max_batch, max_batch_capacity, max_seq_len, num_gpu, pad_idx):
        self.batches = []
        budget = max_batch_capacity * 1000000
        src, dst, sl, dl, lex = [], [], [], [], []  # lex: one row of proposals per sentence, drawn from its source (:113-115)
        max_s = max_t = 0
        for ex in examples:
            s = torch.LongTensor(list(ex[0][:max_seq_len]))
            t = torch.LongTensor(list(ex[1][:max_seq_len]))
            new_s, new_t, n = max(max_s, s.numel()), max(max_t, t.numel()), len(src) + 1
            over = (new_s + new_t) * n > max_batch or (new_s ** 2 + new_t ** 2) * n * new_t > budget
            if over and len(src) >= num_gpu and n > 1:
                self._emit(src, dst, sl, dl, pad_idx, lex)
                src, dst, sl, dl, lex = [], [], [], [], []
                new_s, new_t = s.numel(), t.numel()
            src.append(s); dst.append(t); sl.append(ex[2]); dl.append(ex[3])
            if self.lex_dict is not None:
                lex.append(get_lex_suggestions(self.lex_dict, s, pad_idx))
            max_s, max_t = new_s, new_t
        if len(src) > 0 and len(src) >= num_gpu:
            self._emit(src, dst, sl, dl, pad_idx, lex)

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, item):
        return self.batches[item]


class MassDataset(Dataset):
    def __init__(self, batch_pickle_dir: Optional[str], max_batch_capacity: int, max_batch: int, pad_idx: int,
                 max_seq_len: int = 512, keep_examples: bool = False, example_list: Optional[List] = None, lex_dict=None,
                 keep_pad_idx: bool = True, ngpu: int = 1):
        self.lex_dict = lex_dict
        self.keep_pad_idx = keep_pad_idx
        self.ngpu = ngpu
        if example_list is None:
            self.examples_list = [self.read_example_file(path) for path in sorted(glob.glob(batch_pickle_dir + "*"))]
        else:
            self.examples_list = example_list
        self.batch_items(max_batch, max_batch_capacity, max_seq_len, pad_idx)
        if example_list is None and not keep_examples:
            self.examples_list = []

    @staticmethod
    def read_example_file(path):
        with open(path, "rb") as fr:
            return marshal.load(fr)

    def batch_items(self, max_batch, max_batch_capacity, max_seq_len, pad_idx):
        self.batches = []
        self.lang_ids = set()
        budget = max_batch_capacity * 1000000
        groups = []
        cur, langs, lex, longest = [], [], [], 0  # lex: proposals drawn from the sentence itself (:230-232)
        for examples in self.examples_list:
            for ex in examples:
                if len(ex[0]) > max_seq_len:
                    continue
                ids = list(ex[0])
                self.lang_ids.add(int(ids[0]))
                new_longest, n = max(longest, len(ids)), len(cur) + 1
                over = 2 * new_longest * n > max_batch or 2 * new_longest ** 3 * n > budget
                if over and len(cur) >= self.ngpu and n > 1:
                    groups.append((cur, langs, lex))
                    cur, langs, lex, new_longest = [], [], [], len(ids)
                cur.append(ids); langs.append(ex[1])
                if self.lex_dict is not None:
                    lex.append(get_lex_suggestions(self.lex_dict, ids, pad_idx))
                longest = new_longest
        if len(cur) > 0 and len(cur) >= self.ngpu:
            groups.append((cur, langs, lex))
        for sents, lg, lx in groups:
            texts = pad_sequence([torch.LongTensor(s) for s in sents], batch_first=True, padding_value=pad_idx)
            proposal = _pad_proposals(lx, pad_idx) if self.lex_dict is not None else torch.LongTensor([pad_idx])
            self.batches.append({"src_texts": texts, "langs": torch.LongTensor(lg), "proposal": proposal,
                                 "pad_idx": _first_pad_index(texts, pad_idx)})

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, item):
        return self.batches[item]


# ------------------------------------------------------------------------------------------- image / caption data
# What the reference computes from pixels on every batch with a frozen torchvision ResNet (``ModifiedResnet`` up to
# ``x8.view().permute()``, src/image_model.py:24-36) is a constant of the image: it is computed once, by
# ``python -m imagetranslate_amd.extract_features`` (resnet.ResNetTrunk on the MFMA convolution kernels), and enters here as
# pre-extracted region features.  A feature directory holds ``features.pt`` = torch.save({"paths": [str, ...],
# "feats": Tensor[n_images, regions, C]}) (read with ``weights_only=True``).  The caption file is the reference's own:
# marshal of (unique_images: {image id: path}, captions: [(image id, caption ids), ...]) (src/dataset.py:301-306).
# Optionally, the frozen Faster-RCNN's output (src/image_model.py:44-82) enters the same way: "obj_feats" [n_images, M, 1024]
# (box features), "obj_boxes" [n_images, M, 4] (x1, y1, x2, y2 in pixels of the detector's 800-pixel frame) and "obj_labels"
# [n_images, M] int64 in [0, 91), real detections first, label 0 = padding.  Batches then carry batch["objects"] =
# {"feats", "boxes", "labels"} trimmed to the batch's largest real count (the reference pads to the batch maximum, :53-57);
# a batch without a single detection carries no "objects" (no object stream, :53).
class RegionFeatures:
    def __init__(self, root_img_dir: str):
        import os
        blob = torch.load(os.path.join(root_img_dir, "features.pt"), map_location="cpu", weights_only=True)
        self.paths = list(blob["paths"])
        self.feats = blob["feats"]
        assert self.feats.dim() == 3 and self.feats.size(0) == len(self.paths), "features.pt: feats must be [n_images, regions, C]"
        self.index = {p: i for i, p in enumerate(self.paths)}
        self.obj_feats, self.obj_boxes, self.obj_labels = blob.get("obj_feats"), blob.get("obj_boxes"), blob.get("obj_labels")
        if self.obj_labels is not None:
            M = self.obj_labels.size(1)
            assert self.obj_labels.dim() == 2 and self.obj_labels.size(0) == len(self.paths), "features.pt: obj_labels must be [n_images, M]"
            assert tuple(self.obj_feats.shape) == (len(self.paths), M, 1024), "features.pt: obj_feats must be [n_images, M, 1024]"
            assert tuple(self.obj_boxes.shape) == (len(self.paths), M, 4), "features.pt: obj_boxes must be [n_images, M, 4]"
            self.obj_labels = self.obj_labels.long()
            assert M == 0 or (int(self.obj_labels.min()) >= 0 and int(self.obj_labels.max()) < 91), "features.pt: obj_labels outside [0, 91)"

    def get_objects(self, paths):
        """batch["objects"] for these images, trimmed to their largest real detection count, or None (no object keys in
        features.pt, or no detection in any of these images)."""
        if self.obj_labels is None:
            return None
        rows = [self.index.get(p, -1) for p in paths]
        labels = self.obj_labels[[max(r, 0) for r in rows]].clone()
        for k, r in enumerate(rows):
            if r < 0:
                labels[k].zero_()
        real = labels != 0
        n = int((real.long() * torch.arange(1, labels.size(1) + 1)).max()) if labels.numel() else 0  # last real column + 1
        if n == 0:
            return None
        idx = [max(r, 0) for r in rows]
        return {"feats": self.obj_feats[idx, :n].float().clone(), "boxes": self.obj_boxes[idx, :n].float().clone(),
                "labels": labels[:, :n].contiguous()}

    def get(self, paths) -> torch.Tensor:
        """[len(paths), regions, C]; an image without features gets zeros (the reference substitutes a black image, :367)."""
        rows = [self.index.get(p, -1) for p in paths]
        out = self.feats[[max(r, 0) for r in rows]].clone()
        for k, r in enumerate(rows):
            if r < 0:
                out[k].zero_()
        return out


def _with_objects(batch, features, paths):
    objects = features.get_objects(paths) if hasattr(features, "get_objects") else None
    if objects is not None:
        batch["objects"] = objects
    return batch


class ImageCaptionDataset(Dataset):
    """src/dataset.py:278-376 with region features in place of pixels: captions in file order, a batch closed when it
    would hold more than ``max_img_per_batch`` images or 2 * L^3 * n > max_capacity * 1e6 (L = longest caption).
    ``use_neg_samples`` (the reference's ImageCaptionDatasetwNegSamples, :385-398): every item also carries ``"neg"``, the
    same min(number of captions, max(30, batch size)) captions for all rows of the batch, sampled without replacement from
    all captions and padded with pad_idx, and ``"neg_mask"``.  They are drawn from a generator of the dataset's own
    (``neg_seed``), not from the global ``random`` state: a seed pins the draws and nothing else is disturbed."""

    def __init__(self, root_img_dir: str, data_bin_file: str, max_capacity: int, text_processor, max_img_per_batch: int,
                 lex_dict=None, ngpu: int = 1, use_neg_samples: bool = False, features: Optional[RegionFeatures] = None,
                 neg_seed: int = 0):
        self.lex_dict = lex_dict
        self.ngpu = ngpu
        self.use_neg_samples = bool(use_neg_samples)
        self._neg_rng = random.Random(neg_seed)
        self.pad_idx = text_processor.pad_token_id()
        self.features = features if features is not None else RegionFeatures(root_img_dir)
        self.batches, self.image_batches, self.all_captions, self.lang_ids = [], [], [], set()
        self.proposal_batches = []  # per batch [B, Pmax] proposals drawn from the captions (:314-316), None without --dict
        budget = max_capacity * 1000000
        with open(data_bin_file, "rb") as fp:
            self.unique_images, captions = marshal.load(fp)
        tag = text_processor.id2token(captions[0][1][0])
        self.lang_ids.add(int(captions[0][1][0]))
        self.lang = text_processor.languages[tag] if tag in text_processor.languages else 0
        cur, imgs, lex, longest = [], [], [], 0
        for image_id, caption in captions:
            if str(self.unique_images[image_id]).lower().endswith(".png"):
                continue
            cap = torch.LongTensor(list(caption))
            self.all_captions.append(cap)
            cur.append(cap); imgs.append(image_id)
            if lex_dict is not None:
                lex.append(get_lex_suggestions(lex_dict, cap, self.pad_idx))
            longest = max(longest, cap.numel())
            over = len(imgs) > max_img_per_batch or 2 * longest ** 3 * len(cur) > budget
            if over and len(cur) - 1 >= self.ngpu and len(cur) > 1:
                self._emit(cur[:-1], imgs[:-1], lex[:-1])
                cur, imgs, lex = [cur[-1]], [imgs[-1]], lex[-1:]  # the sentence that did not fit carries its proposals over (:328)
                longest = cur[0].numel()
        if cur:
            self._emit(cur, imgs, lex)

    def _emit(self, caps, imgs, lex):
        texts = pad_sequence(caps, batch_first=True, padding_value=self.pad_idx)
        self.batches.append((texts, texts != self.pad_idx, _first_pad_index(texts, self.pad_idx)))
        self.image_batches.append(list(imgs))
        self.proposal_batches.append(_pad_proposals(lex, self.pad_idx) if self.lex_dict is not None else None)

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, item):
        texts, mask, pad_indices = self.batches[item]
        paths = [self.unique_images[i] for i in self.image_batches[item]]
        out = {"images": self.features.get(paths), "captions": texts, "pad_idx": pad_indices,
               "langs": torch.LongTensor([self.lang] * texts.size(0)), "caption_mask": mask,
               "proposal": self.proposal_batches[item]}
        if self.use_neg_samples:
            n = min(len(self.all_captions), max(30, int(texts.size(0))))
            out["neg"] = pad_sequence(self._neg_rng.sample(self.all_captions, n), batch_first=True, padding_value=self.pad_idx)
            out["neg_mask"] = out["neg"] != self.pad_idx
        return _with_objects(out, self.features, paths)


class ImageCaptionTestDataset(ImageCaptionDataset):
    """src/dataset.py:396-421: one row per distinct image of the batch, its captions kept as references."""

    def __getitem__(self, item):
        texts, _, _ = self.batches[item]
        refs, order = {}, []
        for row, image_id in enumerate(self.image_batches[item]):
            if image_id not in refs:
                refs[image_id] = []
                order.append(image_id)
            cap = texts[row]
            refs[image_id].append(cap)
        max_len = int(texts.size(1))
        first_tokens = torch.LongTensor([int(refs[i][0][0]) for i in order])
        paths = [self.unique_images[i] for i in order]
        out = {"images": self.features.get(paths), "img_ids": order, "captions": refs, "first_tokens": first_tokens,
               "langs": torch.LongTensor([self.lang] * len(order)), "max_len": max_len + 10, "proposal": None}
        return _with_objects(out, self.features, paths)


class ImageDataset(Dataset):
    """src/dataset.py:424-476 (inference): every image of the feature directory, ``max_img_per_batch`` per batch."""

    def __init__(self, root_img_dir: str, max_img_per_batch: int, target_lang: int, first_token: int,
                 features: Optional[RegionFeatures] = None):
        self.target_lang, self.first_token = target_lang, first_token
        self.features = features if features is not None else RegionFeatures(root_img_dir)
        paths = [p for p in self.features.paths if not p.lower().endswith(".png")]
        self.image_batches = [paths[i:i + max_img_per_batch] for i in range(0, len(paths), max_img_per_batch)]

    def __len__(self):
        return len(self.image_batches)

    def __getitem__(self, item):
        paths = self.image_batches[item]
        out = {"images": self.features.get(paths), "tgt_langs": torch.LongTensor([self.target_lang] * len(paths)),
               "first_tokens": torch.LongTensor([self.first_token] * len(paths)), "paths": paths}
        return _with_objects(out, self.features, paths)
