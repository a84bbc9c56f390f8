"""Text-to-image-embedding trainer -- counterpart of src/train_txt2image.py (``Caption2ImageTrainer.train_epoch`` ``:42-115``,
``eval`` ``:117-144``, ``train`` ``:147-194``): a trained, frozen ``ImageCaptioning`` model (``--pretrained``) turns the region
features of every image into its 49 x d embedding (eval mode, no gradient), and ``Caption2Image`` learns to predict that
embedding from the caption: L2 distance over the batch divided by the number of images.  The model step is the HIP path
(``Caption2Image.loss_fused``: encoder stack, fused dropout + pooling, linear layer, ``imt_l2_dist``), then the clip + Adam
step of the other trainers.  Checkpoints (``<model>.latest``) hold weights only: no pickled optimizer (``--save-opt`` is
refused); with ``--save-state`` the student's ``train_state.pt`` (checkpoint.py) goes beside them and ``--resume DIR`` continues from
it -- the frozen captioner is reloaded from ``--pretrained`` as ever.  One process, one GPU."""
import os
import random

import torch

from . import dataset
from .image_model import Caption2Image, ImageCaptioning
from .option_parser import get_img_options_parser
from .seq2seq import Seq2Seq
from .textprocessor import TextProcessor
from .trainer import Trainer, add_resume_options, reject_off_path
from .utils import build_optimizer


class Caption2ImageTrainer(Trainer):
    unit = "Image"

    def __init__(self, model, caption_model, **kw):
        super().__init__(model, **kw)
        if self.world_size > 1:
            raise NotImplementedError("Caption2Image trains in one process on one GPU")
        self.caption_model = caption_model.eval()

    @torch.no_grad()
    def image_encoding(self, batch):
        """[B, 49, d] embeddings of the batch's images by the frozen captioner (src/train_txt2image.py:62-64)."""
        self.caption_model.eval()
        return self.caption_model(batch=batch, encode_only=True)

    def txt2image_step(self, batch, accum: int = 1):
        target = self.image_encoding(batch)
        loss, n = self.model.loss_fused(batch["captions"], batch["caption_mask"], batch["langs"], target)
        loss.backward()
        self._finish_micro_step(accum)
        return loss.detach(), n

    @torch.no_grad()
    def dev_loss(self, img_dev_data):
        """sum of the batch losses / number of images (src/train_txt2image.py:117-144)."""
        self.model.eval()
        losses, images = [], 0
        for i in range(len(img_dev_data)):
            batch = img_dev_data[i]
            loss, n = self.model.loss_fused(batch["captions"], batch["caption_mask"], batch["langs"], self.image_encoding(batch))
            losses.append(loss)
            images += n
        self.model.train()
        return float(torch.stack(losses).sum()) / max(images, 1) if losses else 0.0

    def train_epoch(self, img_data, img_dev_data=None, step: int = 0, max_step: int = 300000, save_path: str = None,
                    accum: int = 1, log_every: int = 50, save_every: int = 10000, eval_every: int = 5000, **kwargs):
        def step_fn(kind, i, step):
            loss, n = self.txt2image_step(img_data[i], accum)
            return loss / n, n  # the reference logs sum(loss) / sum(images) (:70-85): the meter weighs by n, so it is fed loss / n

        def after_step(step):
            if save_path and step % save_every == 0:
                self.save_latest(save_path)
            if img_dev_data is not None and step % eval_every == 0:
                print("Dev Loss:", self.dev_loss(img_dev_data), flush=True)

        self.track_dataset(img_data)
        self.track_dataset(img_dev_data)
        start = self.take_resume_pos()
        return self.run_epoch(self.epoch_order([("img", len(img_data))]), step_fn, step=step, max_step=max_step,
                              log_every=log_every, after_step=after_step, start=start)

    @staticmethod
    def train(options):
        reject_off_path(options)
        if getattr(options, "resume_dir", None) and not os.path.isfile(os.path.join(options.resume_dir, "train_state.pt")):
            raise FileNotFoundError("--resume %s: no train_state.pt there" % options.resume_dir)
        if not options.pretrained_path:
            raise ValueError("--pretrained: the directory of the trained ImageCaptioning model is required")
        random.seed(options.seed)
        torch.manual_seed(options.seed)
        tp = TextProcessor(options.tokenizer_path)
        assert tp.pad_token_id() == 0
        caption_model = Seq2Seq.load(ImageCaptioning, options.pretrained_path, tok_dir=options.tokenizer_path,
                                     use_obj=not options.no_obj)
        # --resume DIR holds the STUDENT's snapshot only; the frozen captioner comes from --pretrained as ever.  The student is
        # built from the flags (the snapshot carries its weights and refuses another layout)
        model = Caption2Image(text_processor=tp, enc_layer=options.encoder_layer, embed_dim=options.embed_dim,
                              intermediate_dim=options.intermediate_layer_dim, num_attention_heads=options.heads)
        return Caption2ImageTrainer.run(options, model, caption_model, tp)

    @staticmethod
    def run(options, model, caption_model, tp, features=None):
        """The training loop of ``train`` on models that are already built (``features``: a ``dataset.RegionFeatures``)."""
        dtype = torch.float32 if options.fp32 else torch.bfloat16
        caption_model = caption_model.set_compute_dtype(dtype).cuda().eval()
        model = model.set_compute_dtype(dtype).cuda().train()
        if model.config.hidden_size != caption_model.config.hidden_size:
            raise ValueError("--embed %d: the captioner's embeddings have %d dimensions" % (model.config.hidden_size,
                                                                                          caption_model.config.hidden_size))
        optimizer = build_optimizer(model, options.learning_rate, options.warmup)
        trainer = Caption2ImageTrainer(model=model, caption_model=caption_model, optimizer=optimizer, clip=options.clip,
                                       seed=options.seed)
        feats = features if features is not None else dataset.RegionFeatures(options.image_dir)
        mk = lambda path: dataset.ImageCaptionDataset(root_img_dir=options.image_dir, data_bin_file=path,
                                                      max_capacity=options.img_capacity, text_processor=tp,
                                                      max_img_per_batch=options.max_image, features=feats)
        img_train = mk(options.train_path)
        img_dev = mk(options.dev_path) if options.dev_path else None
        print("image batches", len(img_train), flush=True)
        step = trainer.begin_run(options, getattr(options, "resume_dir", None))
        while options.step > 0 and step < options.step and trainer.epochs_begun < options.num_epochs:
            print("train epoch", trainer.epochs_begun + 1, flush=True)
            step = trainer.train_epoch(img_data=img_train, img_dev_data=img_dev, step=step, max_step=options.step,
                                       save_path=options.model_path, accum=options.accum, log_every=options.log_steps,
                                       save_every=options.save_steps, eval_every=options.eval_steps)
        if options.model_path:
            trainer.save_latest(options.model_path)
        trainer.finish_snapshots()
        if img_dev is not None:
            print("Dev Loss:", trainer.dev_loss(img_dev), flush=True)
        return trainer


def main(argv=None):
    options, _ = add_resume_options(get_img_options_parser()).parse_args(argv)
    Caption2ImageTrainer.train(options)
    print("Finished Training!")


if __name__ == "__main__":
    main()
