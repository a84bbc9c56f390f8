"""Masked-LM pre-training -- counterpart of src/train_lm.py (``LMTrainer.train_epoch`` ``:45-108``, ``validate_and_save``
``:110-138``, ``train`` ``:146-190``): batches of ``--batch`` rows of the ``create_batches`` blocks in file order, BERT masking on
the device (``imt_mlm_mask``: one launch in front of the encoder, its count restated on the host so that nothing is read back),
``LM.loss_fused``, then the clip + Adam step of the other trainers.  The dataset's tensors are never modified -- every step masks
a device copy -- so there is no unmask.  The mask of a step is drawn from (--seed, step) alone: a resumed run masks as the
uninterrupted one would.  The dev loss masks batch b from (--seed, b), the same way every time (the reference redraws, so its
successive dev losses are not comparable); its best value saves to ``--model``, the latest weights go to ``<model>.latest``.
Checkpoints hold weights, config and tokenizer: no pickled optimizer (``--cont`` is refused; ``--save-state`` / ``--resume``
continue a run).  ``--reformer`` is not built.  One process, one GPU."""
import os
import random

import torch

from .dataset import TextCollator, TextDataset
from .lm import LM
from .option_parser import get_lm_option_parser
from .textprocessor import TextProcessor
from .trainer import Trainer, add_resume_options, resume_dir_of
from .utils import build_optimizer, mask_text_count, mask_text_device


def mask_seed(seed: int, index: int, dev: bool = False) -> int:
    """Seed of the masking kernel for training step ``index`` (or dev batch ``index``): from a generator seeded by (seed, index,
    dev) alone, as ``train_txt_sim.draw_negative`` draws -- the same whatever came before."""
    return random.Random((int(seed) * 1000003 + int(index)) * 2 + int(bool(dev))).getrandbits(63)


class TextBatches:
    """``TextDataset`` rows in file order as collated batches of ``batch`` rows (the reference's DataLoader with shuffle=False,
    src/train_lm.py:181-184): item i is {"texts", "pad_mask", "langs"} of rows [i * batch, (i + 1) * batch)."""

    def __init__(self, data: TextDataset, batch: int, pad_idx: int):
        self.data, self.batch, self.collate = data, max(1, int(batch)), TextCollator(pad_idx)

    def __len__(self):
        return (len(self.data) + self.batch - 1) // self.batch

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self.collate([self.data[j] for j in range(i * self.batch, min(len(self.data), (i + 1) * self.batch))])


class LMTrainer(Trainer):
    unit = "Tokens"  # masked tokens

    def __init__(self, model, mask_prob: float = 0.15, **kw):
        if int(kw.get("world_size", 1)) > 1:
            raise NotImplementedError("the masked LM trains in one process on one GPU")
        super().__init__(model, **kw)
        self.mask_prob = mask_prob

    @staticmethod
    def config_dropout(model, dropout: float):
        """--dropout into the encoder's config (src/train_lm.py:140-143); the stack's descriptor is rebuilt from it."""
        model.encoder.config.hidden_dropout_prob = dropout
        model.encoder.config.attention_probs_dropout_prob = dropout
        model.encoder.__dict__.pop("_imt_desc_cache", None)

    def masked_loss(self, batch, seed: int):
        """(loss, n) of one batch masked with ``seed``; n == 0: nothing was masked and nothing was launched."""
        tp = self.model.text_processor
        n = mask_text_count(self.mask_prob, batch["pad_mask"], batch["texts"], tp, seed)
        if n == 0:
            return torch.zeros((), device=self.model._device), 0
        device = self.model._device
        texts = batch["texts"].to(device=device, dtype=torch.int64, copy=True).contiguous()
        pads = batch["pad_mask"].to(device)
        masked = mask_text_device(self.mask_prob, pads, texts, tp, seed, count=n)
        return self.model.loss_fused(masked["texts"], pads, batch["langs"], masked["idx"], masked["targets"])

    def lm_step(self, batch, step: int, accum: int = 1):
        loss, n = self.masked_loss(batch, mask_seed(self.seed, step))
        if n == 0:  # nothing to predict (src/train_lm.py:61-62): not a step
            return loss, 0
        loss.backward()
        self._finish_micro_step(accum)
        return loss.detach(), n

    @torch.no_grad()
    def dev_loss(self, dev_data):
        """Token-weighted mean of the dev batches' losses in eval mode; batch b is masked from (seed, b) every time."""
        self.model.eval()
        losses, counts = [], []
        for b in range(len(dev_data)):
            loss, n = self.masked_loss(dev_data[b], mask_seed(self.seed, b, dev=True))
            if n:
                losses.append(loss)
                counts.append(n)
        self.model.train()
        if not losses:
            return 0.0
        w = torch.tensor(counts, dtype=torch.float32, device=losses[0].device)
        return float((torch.stack(losses).float() * w).sum() / w.sum())

    def train_epoch(self, data, dev_data=None, step: int = 0, max_step: int = 125000, save_path: str = None, accum: int = 1,
                    log_every: int = 50, save_every: int = 500, eval_every: int = 500, **kwargs):
        def step_fn(kind, i, step):  # `step` is the count before this batch: the mask is drawn from it
            return self.lm_step(data[i], step, accum)

        def after_step(step):
            if save_path and step % save_every == 0:
                self.save_latest(save_path)
            if dev_data is not None and step % eval_every == 0:
                self.validate_and_save(dev_data, save_path)

        start = self.take_resume_pos()
        order = [("lm", i) for i in range(len(data))]  # file order, as the reference reads it (and as the block cache likes it)
        return self.run_epoch(order, step_fn, step=step, max_step=max_step, log_every=log_every, after_step=after_step,
                              skip_empty=True, start=start)

    def validate_and_save(self, dev_data, save_path):
        dl = self.dev_loss(dev_data)
        print("Current dev loss", dl, flush=True)
        if dl < self.best_loss:  # src/train_lm.py:129
            self.best_loss = dl
            if save_path:
                print("saving best dev loss", dl, flush=True)
                self.model.save(save_path)
        return dl

    @staticmethod
    def train(options):
        if options.reformer:
            raise NotImplementedError("--reformer: ReformerLM is not built")
        if options.continue_train:
            raise NotImplementedError("--cont: a pickled optimizer is never loaded; use --pretrained to continue from saved weights, "
                                      "or --save-state / --resume to continue a run with its optimizer state")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise NotImplementedError("the masked LM trains in one process on one GPU (WORLD_SIZE=%s)" % os.environ["WORLD_SIZE"])
        if not options.train_path:
            raise ValueError("--train is required")
        resume = resume_dir_of(options)  # --resume DIR: the model is built from DIR as --pretrained builds it
        random.seed(options.seed)
        torch.manual_seed(options.seed)
        if resume or options.pretrained_path:
            model = LM.load(resume or options.pretrained_path)
        else:
            if not options.tokenizer_path:
                raise ValueError("--tok is required without --pretrained")
            model = LM(text_processor=TextProcessor(options.tokenizer_path), enc_layer=options.encoder_layer,
                       embed_dim=options.embed_dim, intermediate_dim=options.intermediate_layer_dim,
                       num_attention_heads=options.heads)
        return LMTrainer.run(options, model, resume)

    @staticmethod
    def run(options, model, resume=None):
        """The training loop of ``train`` on a model that is already built."""
        LMTrainer.config_dropout(model, options.dropout)
        model = model.set_compute_dtype(torch.float32 if options.fp32 else torch.bfloat16).cuda().train()
        optimizer = build_optimizer(model, options.learning_rate, options.warmup)
        trainer = LMTrainer(model=model, mask_prob=options.mask_prob, optimizer=optimizer, clip=options.clip, seed=options.seed)
        pad = model.text_processor.pad_token_id()
        train = TextBatches(TextDataset(save_cache_dir=options.train_path, max_cache_size=options.cache_size), options.batch, pad)
        dev = None
        if options.dev_path:
            dev = TextBatches(TextDataset(save_cache_dir=options.dev_path, max_cache_size=options.cache_size, load_all=True),
                              options.batch, pad)
        if not len(train):
            raise ValueError("no batches in %s" % options.train_path)
        print("LM batches", len(train), "dev batches", len(dev) if dev is not None else 0, flush=True)
        step = trainer.begin_run(options, resume)
        while options.step > 0 and step < options.step and trainer.epochs_begun < options.num_epochs:
            print("train epoch", trainer.epochs_begun + 1, flush=True)
            step = trainer.train_epoch(train, dev_data=dev, step=step, max_step=options.step, save_path=options.model_path,
                                       accum=options.accum, log_every=options.log_steps, save_every=options.save_steps,
                                       eval_every=options.eval_steps)
        if options.model_path:
            trainer.save_latest(options.model_path)
        trainer.finish_snapshots()
        if dev is not None:
            trainer.validate_and_save(dev, options.model_path)
        return trainer


def get_options_parser():
    """The flags of src/train_lm.py (``get_lm_option_parser``) with --save-state / --resume; ``accum`` (which the snapshot code
    reads) is a default of this parser, 1, not a flag: the reference's LM trainer has none."""
    parser = add_resume_options(get_lm_option_parser())
    parser.set_defaults(accum=1)
    return parser


def main(argv=None):
    options, _ = get_options_parser().parse_args(argv)
    LMTrainer.train(options)
    print("Finished Training!")


if __name__ == "__main__":
    main()
