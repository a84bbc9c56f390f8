"""Sentence-similarity trainer -- counterpart of src/train_txt_sim.py (``SenSimTrainer.train_epoch`` ``:24-118``, ``eval``
``:120-153``, ``train`` ``:155-205``): sentence pairs from ``--train_mt``, one batch of monolingual negatives per side from
``--src-neg`` / ``--dst-neg`` each step, the two-sided contrastive loss of ``SenSim`` (encoder stack x 4, fused pooling,
``imt_sensim_loss``), then the clip + Adam step of the other trainers.  The dev loss (``--dev_mt``) is the one-sided loss without
negatives; its best value saves to ``--model``, the latest weights go to ``<model>.latest``.  Checkpoints hold weights only: no
pickled optimizer (``--save-opt`` is refused); with ``--save-state`` ``train_state.pt`` (checkpoint.py) goes beside them and ``--resume
DIR`` continues from it (the negatives are drawn from (seed, step): they continue with the step count).  One process, one GPU."""
import os
import random

import torch

from . import dataset
from . import hip_ops as O
from .option_parser import get_img_options_parser
from .sen_sim import SenSim
from .seq2seq import Seq2Seq
from .textprocessor import TextProcessor
from .trainer import Trainer, add_resume_options, batches_from, reject_off_path
from .utils import build_optimizer

NEG_FACTOR = 5  # the negatives' batch and capacity are five times the pairs' (src/train_txt_sim.py:181-182)


def draw_negative(seed: int, step: int, side: int, n_batches: int) -> int:
    """Index of the negative batch of ``side`` (0: source, 1: target) at ``step``: uniform over the side's batches, from a
    generator seeded by (seed, step, side) alone -- the reference takes the first batch of a freshly shuffled loader
    (``next(iter(loader))``, :50,55), a uniform draw too.  The same seed and step give the same index whatever came before."""
    return random.Random((int(seed) * 1000003 + int(step)) * 2 + int(side)).randrange(n_batches)


def load_language_model(directory: str, tok_dir: str):
    """The model ``--pretrained DIR`` names: a masked language model when DIR holds ``config`` (what ``LM.save`` writes), a
    ``Seq2Seq`` when it holds ``mt_config``.  ``SenSim.init_from_lm`` reads only its ``.encoder``."""
    if os.path.isfile(os.path.join(directory, "config")):
        from .lm import LM
        return LM.load(directory)
    return Seq2Seq.load(Seq2Seq, directory, tok_dir=tok_dir)


class SenSimTrainer(Trainer):
    unit = "Sentences"

    def __init__(self, model, **kw):
        if int(kw.get("world_size", 1)) > 1:
            raise NotImplementedError("SenSim trains in one process on one GPU")
        super().__init__(model, **kw)

    def negatives(self, data, step: int, side: int, n_pairs: int):
        """(inputs, mask, langs) of this step's negative batch, cut to what one loss call takes beside the pairs."""
        batch = data[draw_negative(self.seed, step, side, len(data))]
        keep = O.CONTRASTIVE_MAX_N - n_pairs
        texts, langs = batch["src_texts"][:keep], batch["langs"][:keep]
        return texts, texts != self.model.text_processor.pad_token_id(), langs

    def sim_step(self, batch, src_neg, dst_neg, step: int, accum: int = 1):
        n = int(batch["src_texts"].size(0))
        sn, sm, sl = self.negatives(src_neg, step, 0, n)
        tn, tm, tl = self.negatives(dst_neg, step, 1, n)
        loss, n = self.model.loss_fused(batch["src_texts"], batch["src_pad_mask"], batch["src_langs"], batch["dst_texts"],
                                        batch["dst_pad_mask"], batch["dst_langs"], src_neg_inputs=sn, src_neg_mask=sm,
                                        src_neg_langs=sl, tgt_neg_inputs=tn, tgt_neg_mask=tm, tgt_neg_langs=tl)
        loss.backward()
        self._finish_micro_step(accum)
        return loss.detach(), n

    @torch.no_grad()
    def dev_loss(self, dev_data):
        """Sentence-weighted mean of the batches' one-sided losses (src/train_txt_sim.py:120-144: no negatives)."""
        self.model.eval()
        losses, counts = [], []
        for batch in dev_data:
            loss, n = self.model.loss_fused(batch["src_texts"], batch["src_pad_mask"], batch["src_langs"], batch["dst_texts"],
                                            batch["dst_pad_mask"], batch["dst_langs"])
            losses.append(loss)
            counts.append(n)
        self.model.train()
        if not losses:
            return 0.0
        w = torch.tensor(counts, dtype=torch.float32, device=losses[0].device)
        return float((torch.stack(losses) * w).sum() / w.sum())

    def train_epoch(self, mt_data, src_neg, dst_neg, dev_data=None, step: int = 0, max_step: int = 300000, save_path: str = None,
                    accum: int = 1, log_every: int = 50, save_every: int = 500, eval_every: int = 5000, **kwargs):
        def step_fn(kind, i, step):  # `step` is the count before this batch: the negatives are drawn from it
            # the loss is already per sentence (divided by B): the meter weighs it by n (:71-75)
            return self.sim_step(mt_data[i], src_neg, dst_neg, step, accum)

        def after_step(step):
            if save_path and step % save_every == 0:
                self.save_latest(save_path)
            if dev_data is not None and step % eval_every == 0:
                self.validate_and_save(dev_data, save_path)

        start = self.take_resume_pos()
        return self.run_epoch(self.epoch_order([("mt", len(mt_data))]), step_fn, step=step, max_step=max_step,
                              log_every=log_every, after_step=after_step, start=start)

    def validate_and_save(self, dev_data, save_path):
        dl = self.dev_loss(dev_data)
        print("Dev Loss:", dl, flush=True)
        if dl <= self.best_loss:  # :146
            self.best_loss = dl
            if save_path:
                print("Saving best Loss", dl, flush=True)
                self.model.save(save_path)
        return dl

    @staticmethod
    def train(options):
        reject_off_path(options)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise NotImplementedError("SenSim trains in one process on one GPU (WORLD_SIZE=%s)" % os.environ["WORLD_SIZE"])
        for flag, val in (("--train_mt", options.mt_train_path), ("--src-neg", options.src_neg), ("--dst-neg", options.dst_neg)):
            if not val:
                raise ValueError("%s is required" % flag)
        random.seed(options.seed)
        torch.manual_seed(options.seed)
        tp = TextProcessor(options.tokenizer_path)
        assert tp.pad_token_id() == 0
        model = SenSim(text_processor=tp, enc_layer=options.encoder_layer, embed_dim=options.embed_dim,
                       intermediate_dim=options.intermediate_layer_dim, num_attention_heads=options.heads)
        if getattr(options, "resume_dir", None) and not os.path.isfile(os.path.join(options.resume_dir, "train_state.pt")):
            raise FileNotFoundError("--resume %s: no train_state.pt there" % options.resume_dir)
        if options.pretrained_path:  # (--pretrained is a language model here, not a SenSim: --resume does not replace it; the
            # model is built from the flags, the snapshot carries its weights and refuses another layout)
            model.init_from_lm(load_language_model(options.pretrained_path, options.tokenizer_path))
        return SenSimTrainer.run(options, model, tp)

    @staticmethod
    def run(options, model, tp):
        """The training loop of ``train`` on a model that is already built."""
        model = model.set_compute_dtype(torch.float32 if options.fp32 else torch.bfloat16).cuda().train()
        optimizer = build_optimizer(model, options.learning_rate, options.warmup)
        trainer = SenSimTrainer(model=model, optimizer=optimizer, clip=options.clip, seed=options.seed)
        pad = tp.pad_token_id()
        mt_kw = dict(max_batch_capacity=options.total_capacity, max_batch=options.batch, pad_idx=pad, max_seq_len=options.max_seq_len,
                     keep_pad_idx=False)
        mt_train = batches_from(options.mt_train_path, **mt_kw)
        mt_dev = batches_from(options.mt_dev_path, **mt_kw) or None
        neg = lambda path: dataset.MassDataset(batch_pickle_dir=path, max_batch_capacity=options.total_capacity * NEG_FACTOR,
                                               max_batch=options.batch * NEG_FACTOR, pad_idx=pad, keep_pad_idx=False,
                                               max_seq_len=options.max_seq_len, keep_examples=False)
        src_neg, dst_neg = neg(options.src_neg), neg(options.dst_neg)
        if not len(mt_train) or not len(src_neg) or not len(dst_neg):
            raise ValueError("no batches: %d of sentence pairs, %d / %d of negatives" % (len(mt_train), len(src_neg), len(dst_neg)))
        print("MT batches", len(mt_train), "negative batches", len(src_neg), len(dst_neg), "dev batches", len(mt_dev or []), flush=True)
        step = trainer.begin_run(options, getattr(options, "resume_dir", None))
        while options.step > 0 and step < options.step and trainer.epochs_begun < options.num_epochs:
            print("train epoch", trainer.epochs_begun + 1, flush=True)
            step = trainer.train_epoch(mt_train, src_neg, dst_neg, dev_data=mt_dev, step=step, max_step=options.step,
                                       save_path=options.model_path, accum=options.accum, log_every=options.log_steps,
                                       save_every=options.save_steps, eval_every=options.eval_steps)
        if options.model_path:
            trainer.save_latest(options.model_path)
        trainer.finish_snapshots()
        if mt_dev is not None:
            trainer.validate_and_save(mt_dev, options.model_path)
        return trainer


def main(argv=None):
    options, _ = add_resume_options(get_img_options_parser()).parse_args(argv)
    SenSimTrainer.train(options)
    print("Finished Training!")


if __name__ == "__main__":
    main()
