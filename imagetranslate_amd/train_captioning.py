"""Captioning trainer -- counterpart of src/train_captioning.py (``ImageCaptionTrainer.train_epoch`` ``:26-141``,
``train`` ``:194-286``): image batches (region features -> ``fc`` + location embedding -> decoder) and, optionally,
MT batches as a second task whose loss is weighted by ``--mtlw`` (``:83``); gradients of both tasks accumulate, the clip
runs after every backward and the optimizer steps every ``--acc`` micro-steps (``:91-97``).  The model step is the HIP
path (``ImageCaptioning.loss_fused``); when features.pt carries detector output (``obj_*`` keys, dataset.RegionFeatures)
and the model has its object stream (no ``--no-obj``), the batches' ``objects`` train it.  BLEU evaluation needs sacrebleu (absent): the dev set is scored by its loss and,
with ``eval_captions``, decoded with beam search.  ``--save-state`` adds ``train_state.pt`` (checkpoint.py) to ``<model>.latest`` every
``--save-steps`` steps; ``--resume DIR`` continues the run saved there (trainer.py)."""
import datetime
import os
import random

import torch

from . import dataset
from .image_model import ImageCaptioning, ImageMassSeq2Seq
from .option_parser import get_img_options_parser
from .seq2seq import Seq2Seq
from .seq_gen import BeamDecoder, get_outputs_until_eos
from .textprocessor import TextProcessor
from .train_image_mt import ImageMTTrainer
from .trainer import (Trainer, add_resume_options, batches_from, init_distributed, load_lex_dict, reject_off_path, resume_dir_of,
                      use_lex_dict)
from .utils import build_optimizer


class ImageCaptionTrainer(ImageMTTrainer):
    def __init__(self, model, beam_width: int = 5, max_len_a: float = 1.3, max_len_b: int = 5, len_penalty_ratio: float = 0.8,
                 **kw):
        super().__init__(model, **kw)
        self.generator = BeamDecoder(model, beam_width=beam_width, max_len_a=max_len_a, max_len_b=max_len_b,
                                     len_penalty_ratio=len_penalty_ratio)

    # one image batch (src/train_captioning.py:40-58,76-97)
    def caption_step(self, batch, accum: int = 1):
        model, tp = self.model, self.model.text_processor
        # a batch without a single target token is decided on the host BEFORE anything is enqueued; under data parallelism
        # this rank still runs the step's collectives (on its unchanged gradient buffer) and counts the micro-step, so every
        # rank issues the same all-reduces and steps the optimizer at the same time
        if not bool(batch["caption_mask"][:, 1:].any()):
            if self.sync is not None and self.world_size > 1:
                self.sync.begin_step()
                self._finish_micro_step(accum)
            return 0.0, 0
        if self.sync is not None:
            self.sync.begin_step()
        loss, ntokens = model.loss_fused(tgt_inputs=batch["captions"], tgt_mask=batch["caption_mask"], pad_idx=tp.pad_token_id(),
                                         tgt_langs=batch["langs"], batch=batch, proposals=self._proposals(batch))
        loss.backward()
        self._finish_micro_step(accum)
        return loss.detach(), int(ntokens)

    def caption_dev_loss(self, img_dev_data):
        pad = self.model.text_processor.pad_token_id()
        return self._mean_dev_loss(img_dev_data, lambda batch: self.model.loss_fused(
            tgt_inputs=batch["captions"], tgt_mask=batch["caption_mask"], pad_idx=pad, tgt_langs=batch["langs"], batch=batch,
            proposals=self._proposals(batch)))

    @torch.no_grad()
    def eval_captions(self, img_test_data, max_batches: int = None):
        """Beam-search captions of a test dataset (src/train_captioning.py:143-165, without the sacrebleu scoring):
        {image id: caption text}."""
        model, tp = self.model, self.model.text_processor
        model.eval()
        out = {}
        for i in range(len(img_test_data) if max_batches is None else min(max_batches, len(img_test_data))):
            b = img_test_data[i]
            hyps = self.generator(images=b["images"], first_tokens=b["first_tokens"], tgt_langs=b["langs"],
                                  pad_idx=tp.pad_token_id(), max_len=b["max_len"], objects=b.get("objects"),
                                  proposals=self._proposals(b))
            for image_id, h in zip(b["img_ids"], hyps):
                out[image_id] = tp.decode(h[1:].tolist()) if hasattr(tp, "decode") else h[1:].tolist()
        model.train()
        return out

    def train_epoch(self, img_data=None, mt_data=None, img_dev_data=None, mt_dev_data=None, step: int = 0,
                    max_step: int = 300000, save_path: str = None, accum: int = 1, mtl_weight: float = 0.1,
                    log_every: int = 50, eval_every: int = 5000, **kwargs):
        self.track_dataset(img_data)
        self.track_dataset(img_dev_data)  # (its negatives are drawn when a batch is read: the dev loss continues its stream too)
        start = self.take_resume_pos()
        order = Trainer.epoch_order(self, [("img", len(img_data) if img_data is not None else 0), ("mt", len(mt_data or []))])

        def step_fn(kind, i, step):
            if kind == "img":
                return self.caption_step(img_data[i], accum)
            return self.mt_step(mt_data[i], accum, loss_weight=mtl_weight)  # MT data as the second task (:59-75), weighted (:83)

        def after_step(step):  # (without a dev set too: the latest weights are saved)
            if step % eval_every == 0:
                self._validate(img_dev_data, mt_dev_data, save_path)

        return self.run_epoch(order, step_fn, step=step, max_step=max_step, log_every=log_every, after_step=after_step,
                              start=start, skip_empty=True)  # a caption batch without a target token (caption_step) is no step of one process

    log_line = Trainer.log_line  # the reference's "Epoch Step: ..." line, not ImageMTTrainer's

    def _validate(self, img_dev_data, mt_dev_data, save_path):
        score = None
        if img_dev_data is not None:
            score = self.caption_dev_loss(img_dev_data)
            if self.rank == 0:
                print(datetime.datetime.now(), "caption dev loss %.4f (best %.4f)" % (score, self.best_loss), flush=True)
        if mt_dev_data is not None:
            mt = self.dev_loss(mt_dev_data)
            if self.rank == 0:
                print(datetime.datetime.now(), "MT dev loss %.4f" % mt, flush=True)
            score = mt if score is None else score
        if save_path:
            self.save_latest(save_path)
        if self.rank == 0 and save_path:
            if score is not None and score < self.best_loss:
                self.model.save(save_path)
        if score is not None:
            self.best_loss = min(self.best_loss, score)

    @staticmethod
    def train(options):
        reject_off_path(options, lm_supported=True, dict_supported=True)
        resume = resume_dir_of(options)  # --resume DIR: the model is built from DIR as --pretrained builds it
        rank, world = init_distributed()
        random.seed(options.seed)
        torch.manual_seed(options.seed)
        if options.model_path and not os.path.exists(options.model_path):
            os.makedirs(options.model_path, exist_ok=True)
        tp = TextProcessor(options.tokenizer_path)
        assert tp.pad_token_id() == 0
        lex_dict = load_lex_dict(options)
        if resume or options.pretrained_path is not None:
            caption_model = Seq2Seq.load(ImageCaptioning, resume or options.pretrained_path, tok_dir=options.tokenizer_path,
                                         use_obj=not options.no_obj)
        else:
            caption_model = ImageCaptioning(text_processor=tp, tie_embed=options.tie_embed, resnet_depth=options.resnet_depth,
                                            lang_dec=options.lang_decoder, enc_layer=options.encoder_layer,
                                            use_proposals=lex_dict is not None,
                                            dec_layer=options.decoder_layer, embed_dim=options.embed_dim,
                                            intermediate_dim=options.intermediate_layer_dim, use_obj=not options.no_obj,
                                            num_attention_heads=options.heads, image_feat_dim=options.feat_dim)
        if options.lm_path is not None:  # in the reference this is a pretrained MT model whose stacks are adopted (:212-220)
            mt_model = Seq2Seq.load(ImageMassSeq2Seq, options.lm_path, tok_dir=options.tokenizer_path)
            assert len(caption_model.encoder.encoder.layer) == len(mt_model.encoder.encoder.layer)
            assert len(caption_model.decoder.decoder.layer) == len(mt_model.decoder.decoder.layer)
            caption_model.encoder = mt_model.encoder
            caption_model.decoder = mt_model.decoder
            caption_model.output_layer = mt_model.output_layer
        use_lex_dict(caption_model, lex_dict, "train_captioning")
        caption_model.set_compute_dtype(torch.float32 if options.fp32 else torch.bfloat16)
        caption_model = caption_model.cuda().train()
        optimizer = build_optimizer(caption_model, options.learning_rate, options.warmup)
        trainer = ImageCaptionTrainer(model=caption_model, mask_prob=options.mask_prob, optimizer=optimizer, clip=options.clip,
                                      beam_width=options.beam_width, max_len_a=options.max_len_a, max_len_b=options.max_len_b,
                                      len_penalty_ratio=options.len_penalty_ratio, rank=rank, world_size=world, seed=options.seed,
                                      lex_dict=lex_dict)
        feats = dataset.RegionFeatures(options.image_dir)
        mk_img = lambda cls, path: cls(root_img_dir=options.image_dir, data_bin_file=path, max_capacity=options.img_capacity,
                                       text_processor=tp, max_img_per_batch=options.max_image, features=feats,
                                       lex_dict=lex_dict)
        img_train = mk_img(dataset.ImageCaptionDataset, options.train_path)
        img_dev = mk_img(dataset.ImageCaptionDataset, options.dev_path) if options.dev_path else None
        mt_kw = dict(max_batch_capacity=options.total_capacity, max_batch=options.batch, pad_idx=tp.pad_token_id(),
                     max_seq_len=options.max_seq_len, lex_dict=lex_dict)
        mt_train = batches_from(options.mt_train_path, **mt_kw) or None
        mt_dev = batches_from(options.mt_dev_path, **mt_kw) or None
        if rank == 0:
            print("image batches", len(img_train), "MT batches", len(mt_train or []), flush=True)
        step = trainer.begin_run(options, resume)
        while options.step > 0 and step < options.step and trainer.epochs_begun < options.num_epochs:
            step = trainer.train_epoch(img_data=img_train, mt_data=mt_train, img_dev_data=img_dev, mt_dev_data=mt_dev, step=step,
                                       max_step=options.step, save_path=options.model_path, accum=options.accum,
                                       mtl_weight=options.mtl_weight, log_every=options.log_steps, eval_every=options.eval_steps)
        trainer.finish_snapshots()
        trainer._validate(img_dev, mt_dev, options.model_path)
        if rank == 0 and options.model_path and not os.path.exists(os.path.join(options.model_path, "mt_model.state_dict")):
            caption_model.save(options.model_path)
        return trainer


def main(argv=None):
    options, _ = add_resume_options(get_img_options_parser()).parse_args(argv)
    ImageCaptionTrainer.train(options)
    print("Finished Training!")


if __name__ == "__main__":
    main()
