"""Training entry point for the text path -- thin counterpart of src/train_image_mt.py (``ImageMTTrainer``
``:44-333`` and ``train`` ``:394-560``): supervised MT batches and/or MASS batches, label-smoothed loss, gradient
clipping + inverse-sqrt Adam, dev-set loss, best-checkpoint saving, one process per GPU under torch.distributed.
Round 3 adds the back-translation phase (``--fstep`` / ``--langs`` / ``--bt-beam``, src/train_image_mt.py:108-198,509-533): after
``--step`` ordinary steps the optimizer schedule is reset and every monolingual batch is translated by the model itself (KV-cached
beam search, no gradient) and trained on as (translation -> original).  ``--image DIR`` with the caption file of ``--train`` adds
image-caption batches (``:202-237``): per batch ``--mmode`` picks the masked-caption step (the gated text + image branch) or the
contrastive step; back-translation over image batches is not built and refused.  What the reference trainer does around the step that needs
absent packages (apex, sacrebleu, the torchvision image pipeline) is left out; the model step itself is the HIP path.
``--save-state`` writes ``<model>.latest/`` (the model's files, then ``train_state.pt``: checkpoint.py) every ``--save-steps`` steps and at
the end; ``--resume DIR`` builds the model from DIR, restores weights, Adam moments, counters, phase and random streams, and goes on
where the run stopped -- inside the back-translation phase too, without a second schedule reset.  ``--step`` / ``--fstep`` stay totals."""
import datetime
import os
import random
import torch

from torch.nn.utils.rnn import pad_sequence

from . import dataset
from .image_model import ImageMassSeq2Seq
from .option_parser import get_img_options_parser
from .parallel import train_step
from .textprocessor import TextProcessor
from .trainer import (LossMeter, Trainer, add_resume_options, batches_from, init_distributed, load_lex_dict,  # noqa: F401
                      reject_off_path, resume_dir_of, use_lex_dict)
from .utils import build_optimizer, mass_mask_device


class ImageMTTrainer(Trainer):
    def __init__(self, model, mask_prob: float = 0.3, clip: float = 1.0, optimizer=None, rank: int = 0, world_size: int = 1,
                 seed: int = 1234, **kwargs):
        super().__init__(model, optimizer, clip, rank, world_size, seed)
        self.mask_prob = mask_prob
        # MASS span / replacement draws: a generator of this rank's own, so that the ranks' batch ORDER (drawn from a
        # generator every rank seeds identically, Trainer.epoch_order) never depends on how many MASS batches a rank has seen
        self._mass_rng = random.Random((seed + 1) * 7919 + rank)
        # image batches (--mmode): the mixed mode's coin and the masked step's mask_prob ~ U(mask_prob, 1) come from a
        # generator of their own, so that the MASS draws above do not depend on how many image batches a rank has seen
        self.mm_mode = kwargs.get("mm_mode", "mixed")
        if self.mm_mode not in ("mixed", "masked", "contrastive"):
            raise ValueError("--mmode must be mixed, masked or contrastive, got %r" % (self.mm_mode,))
        self._img_rng = random.Random((seed + 2) * 104729 + rank)
        self.image_steps, self.last_image_step = 0, None  # image batches consumed; (kind, loss) of the last one
        self.generator = None  # BeamDecoder of the back-translation phase (built on first use)
        self._pending_searches = None  # generator.searches of a loaded snapshot, until the generator is built
        # "train", or "bt" once the back-translation phase has begun; the step count and the epoch count at which the phase began
        # (its bound is phase_start_step + --fstep) and the bound it ran under
        self.phase, self.phase_start_step, self.phase_epoch0, self.phase_bound = "train", 0, 0, 0
        self.lex_dict = kwargs.get("lex_dict")  # --dict: the back-translation phase looks up proposals for what it generates
        self.bt_kw = dict(beam_width=kwargs.get("bt_beam_width", 1), max_len_a=kwargs.get("max_len_a", 1.3),
                          max_len_b=kwargs.get("max_len_b", 5), len_penalty_ratio=kwargs.get("len_penalty_ratio", 0.8))
        if kwargs.get("bt_sampling", False):  # sampled sources (--bt-sampling): one draw per sentence, this rank's own noise
            self.bt_kw.update(beam_width=1, sampling=True, sampling_topk=kwargs.get("bt_topk", 0),
                              temperature=kwargs.get("bt_temperature", 1.0), nsamples=1, seed=seed + rank)

    # one MT batch (src/train_image_mt.py:239-295)
    def mt_step(self, batch, accum: int = 1, loss_weight: float = 1.0):
        batch = {k: (v[0] if isinstance(v, list) else v) for k, v in batch.items()}
        loss, ntokens = train_step(self.model, self.optimizer, batch, sync=self.sync, clip=self.clip,
                                   update=((self.micro_step + 1) % max(1, accum) == 0), loss_weight=loss_weight)
        self.micro_step += 1  # only a micro-step whose backward ran counts (a failing batch is skipped, train_epoch)
        return loss.detach(), int(ntokens)  # the loss stays on the device: reading it here would stall the host every step

    # one MASS batch (src/train_image_mt.py:186-236): mask a span, recover it with its original positions
    def mass_step(self, batch, accum: int = 1):
        tp = self.model.text_processor
        src = batch["src_texts"].cuda()  # a device copy: the dataset's tensor is never modified, no unmask needed
        masked = mass_mask_device(self.mask_prob, batch["pad_idx"], src, tp, seed=self._mass_rng.getrandbits(62))
        if self.sync is not None:
            self.sync.begin_step()
        loss, ntokens = self.model.loss_fused(src_inputs=masked["src_text"], tgt_inputs=masked["to_recover"],
                                              src_langs=batch["langs"], pad_idx=tp.pad_token_id(),
                                              tgt_positions=masked["positions"], proposals=self._proposals(batch))
        loss.backward()
        self._finish_micro_step(accum)
        return loss.detach(), int(ntokens)

    # one image-caption batch (src/train_image_mt.py:202-237): --mmode picks the masked-caption step (the gated text + image
    # branch) or the contrastive step; "mixed" flips a seeded coin (:207)
    def image_step(self, batch, accum: int = 1):
        batch = {k: (v[0] if isinstance(v, list) else v) for k, v in batch.items()}
        tp = self.model.text_processor
        if self.sync is not None:
            # the gradient exchange is launched layer by layer as the decoder's backward finishes, and the gated branch runs
            # that backward twice: a bucket would leave before the second pass has added to it
            raise NotImplementedError("image batches under data parallelism are not built (one process, one GPU)")
        masked_step = self.mm_mode == "masked" or (self.mm_mode == "mixed" and self._img_rng.random() <= .5)
        if masked_step:
            # "for image masking, we are allowed to mask more than mask_prob" (:212-213)
            mask_prob = min(self._img_rng.uniform(self.mask_prob, 1.0), 1.0 - 1e-6)
            src = batch["captions"].cuda()  # a device copy: the dataset's tensor is never modified
            masked = mass_mask_device(mask_prob, batch["pad_idx"], src, tp, seed=self._img_rng.getrandbits(62))
            loss, ntokens = self.model.loss_fused(src_inputs=masked["src_text"], tgt_inputs=masked["to_recover"],
                                                  tgt_positions=masked["positions"], src_pads=batch["caption_mask"],
                                                  pad_idx=tp.pad_token_id(), src_langs=batch["langs"], tgt_langs=batch["langs"],
                                                  batch=batch, proposals=self._proposals(batch))
        else:  # "nothing to predict" (:274-276): the loss is back-propagated as it is and counts no tokens
            loss, ntokens = self.model.loss_fused(src_inputs=batch["captions"], src_pads=batch["caption_mask"],
                                                  neg_samples=batch["neg"], neg_mask=batch["neg_mask"],
                                                  pad_idx=tp.pad_token_id(), src_langs=batch["langs"], tgt_langs=batch["langs"],
                                                  batch=batch)
        loss.backward()
        self._finish_micro_step(accum)
        self.image_steps += 1
        self.last_image_step = ("masked" if masked_step else "contrastive", loss.detach())
        return loss.detach(), int(ntokens)

    @staticmethod
    def get_lang_dirs(bt_langs: str, text_processor):
        """``--langs en,fa`` -> {token id of <en>: token id of <fa>, and back} (src/train_image_mt.py:535-548); None unless two
        languages are given."""
        langs = {text_processor.token_id("<" + l.strip() + ">") for l in (bt_langs or "").strip().split(",") if l.strip()}
        if len(langs) < 2:
            return None
        assert len(langs) == 2, "back-translation is defined for one language pair (src/train_image_mt.py:541)"
        a, b = sorted(langs)
        return {a: b, b: a}

    # one monolingual batch of the back-translation phase (src/train_image_mt.py:108-198, the is_mass_batch branch): translate the
    # sentences into the other language with the current model (eval mode, no gradient: "we do not backpropagate the data
    # generator following the MASS paper"), then train on (translation -> original)
    def bt_step(self, batch, lang_directions, accum: int = 1):
        from .seq_gen import BeamDecoder
        model, tp = self.model, self.model.text_processor
        pad = tp.pad_token_id()
        src = batch["src_texts"]
        src_mask = src != pad
        first = [int(l) for l in src[:, 0]]
        target_tags = torch.LongTensor([lang_directions[l] for l in first])               # first token of each translation
        dst_langs = torch.LongTensor([tp.languages[tp.id2token(lang_directions[l])] for l in first])
        if self.generator is None:
            self.generator = BeamDecoder(model, **self.bt_kw)
            if self._pending_searches is not None:  # a resumed run's sampled sources continue the saved stream of seeds
                self.generator.searches, self._pending_searches = self._pending_searches, None
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                outs = self.generator(src_inputs=src, src_sizes=batch["pad_idx"], first_tokens=target_tags, src_langs=batch["langs"],
                                      tgt_langs=dst_langs, pad_idx=pad, src_mask=src_mask, unpad_output=False,
                                      beam_width=self.bt_kw["beam_width"], proposals=self._proposals(batch))
        finally:  # a failing search must not leave the model in eval mode
            model.train(was_training)
        outs = [o.cpu() for o in outs]
        translations = pad_sequence(outs, batch_first=True, padding_value=pad)
        translation_proposals = None
        if getattr(model, "use_proposals", False):  # proposals for the generated sources (:157-163)
            if self.lex_dict is None:
                raise ValueError("back-translation with a use_proposals model needs the dictionary (ImageMTTrainer(lex_dict=...))")
            translation_proposals = pad_sequence([dataset.get_lex_suggestions(self.lex_dict, o, pad) for o in outs],
                                                 batch_first=True, padding_value=pad)
        if self.sync is not None:
            self.sync.begin_step()
        loss, ntokens = model.loss_fused(src_inputs=translations, tgt_inputs=src, src_langs=dst_langs, tgt_langs=batch["langs"],
                                         pad_idx=pad, proposals=translation_proposals)
        loss.backward()
        self._finish_micro_step(accum)
        return loss.detach(), int(ntokens)

    @torch.no_grad()
    def _mean_dev_loss(self, data, loss_of):
        """Token-weighted mean of ``loss_of(batch)`` = (loss, ntokens) over data[0..len), in eval mode."""
        self.model.eval()
        total, count = 0.0, 0
        for i in range(len(data)):
            loss, n = loss_of(data[i])
            total += float(loss) * int(n)
            count += int(n)
        self.model.train()
        return total / max(count, 1)

    def dev_loss(self, dev_data):
        return self._mean_dev_loss(dev_data, lambda batch: self.model.loss_fused(
            src_inputs=batch["src_texts"], tgt_inputs=batch["dst_texts"], src_langs=batch["src_langs"],
            tgt_langs=batch["dst_langs"], proposals=self._proposals(batch)))

    # ------------------------------------------------------------------ state that travels (checkpoint.py)
    def begin_phase(self, phase: str, bound: int):
        """The phase that starts now, at this step and epoch count, and runs until ``bound`` steps."""
        self.drop_resume_pos()  # (a snapshot taken on the last step of the phase before: its epoch is not entered again)
        self.phase, self.phase_start_step, self.phase_epoch0, self.phase_bound = phase, int(self.step), int(self.epoch), int(bound)

    def rank_state(self):
        from .trainer import pack_random_state
        out = super().rank_state()
        out["mass_rng"] = pack_random_state(self._mass_rng.getstate())
        out["img_rng"] = pack_random_state(self._img_rng.getstate())
        out["searches"] = self._pending_searches if self.generator is None else int(self.generator.searches)
        return out

    def load_rank_state(self, state):
        from .trainer import unpack_random_state
        super().load_rank_state(state)
        self._mass_rng.setstate(unpack_random_state(state["mass_rng"]))
        self._img_rng.setstate(unpack_random_state(state["img_rng"]))
        if state.get("searches") is not None:
            if self.generator is None:
                self._pending_searches = int(state["searches"])
            else:
                self.generator.searches = int(state["searches"])

    def state_dict(self):
        out = super().state_dict()
        out.update(image_steps=int(self.image_steps), phase=self.phase, phase_start_step=int(self.phase_start_step),
                   phase_epoch0=int(self.phase_epoch0), phase_bound=int(self.phase_bound))
        return out

    def load_state_dict(self, state):
        super().load_state_dict(state)
        self.image_steps = int(state.get("image_steps", 0))
        self.phase, self.phase_bound = str(state.get("phase", "train")), int(state.get("phase_bound", 0))
        self.phase_start_step, self.phase_epoch0 = int(state.get("phase_start_step", 0)), int(state.get("phase_epoch0", 0))

    def epoch_order(self, n_mt: int, n_mass: int, n_img: int = 0):
        """``Trainer.epoch_order`` over this trainer's kinds, concatenated in the order mt, mass, img."""
        return super().epoch_order([("mt", n_mt), ("mass", n_mass), ("img", n_img)])

    def train_epoch(self, mt_data=None, mass_data=None, dev_data=None, step: int = 0, max_step: int = 10 ** 9,
                    save_path: str = None, log_every: int = 50, eval_every: int = 500, accum: int = 1, fine_tune: bool = False,
                    lang_directions=None, img_data=None):
        if fine_tune and img_data is not None and len(img_data) > 0:
            raise NotImplementedError("back-translation over image batches (src/train_image_mt.py:108-198 with is_img_batch) "
                                      "is not built")
        self.track_dataset(img_data)
        start = self.take_resume_pos()
        order = self.epoch_order(len(mt_data or []), len(mass_data or []), len(img_data) if img_data is not None else 0)

        def step_fn(kind, i, step):  # (the contrastive image step reports 0 tokens and still counts as a step)
            if kind == "mt":
                return self.mt_step(mt_data[i], accum)
            if kind == "img":
                return self.image_step(img_data[i], accum)
            if fine_tune:  # back-translation phase: the monolingual batches are translated and trained on (:108-198)
                return self.bt_step(mass_data[i], lang_directions, accum)
            return self.mass_step(mass_data[i], accum)

        def after_step(step):
            if dev_data is not None and step % eval_every == 0:
                self.validate_and_save(dev_data, save_path)

        return self.run_epoch(order, step_fn, step=step, max_step=max_step, log_every=log_every, after_step=after_step, start=start)

    def log_line(self, step, mean, count, secs):
        return "step %d loss %.4f tokens/s %.0f lr %.2e" % (step, mean, count / max(secs, 1e-9), self.optimizer.param_groups[0]["lr"])

    def validate_and_save(self, dev_data, save_path):
        dl = self.dev_loss(dev_data)
        if self.rank == 0:
            print(datetime.datetime.now(), "dev loss %.4f (best %.4f)" % (dl, self.best_loss), flush=True)
            if dl < self.best_loss and save_path:
                self.model.save(save_path)
        self.best_loss = min(self.best_loss, dl)
        return dl


def get_option_parser():
    """The reference's flags (src/option_parser.py:37-88: --train_mt, --dev_mt, --mass_train, --acc, --fp16, --beam ...)
    plus the build's additions (option_parser.py), and on top of them this entry point's own: --bt-sampling / --bt-topk /
    --bt-temperature draw the back-translation phase's sources from the model instead of searching for them."""
    parser = get_img_options_parser()
    parser.add_option("--bt-sampling", action="store_true", dest="bt_sampling", default=False,
                      help="back-translation: sample the sources (seed: --seed + rank)")
    parser.add_option("--bt-topk", dest="bt_topk", type="int", default=0, help="sample among the K best tokens (0: all)")
    parser.add_option("--bt-temperature", dest="bt_temperature", type="float", default=1.0)
    return add_resume_options(parser)


def load_image_data(options, tp, lex_dict=None):
    """--image DIR with the caption file of --train (src/train_image_mt.py:468-473, :636-645): the image-caption batches, or
    None without --image.  DIR must hold a readable features.pt (dataset.RegionFeatures); negative samples are drawn unless
    every image step is a masked one."""
    if not options.image_dir:
        return None
    feats = os.path.join(options.image_dir, "features.pt")
    if not os.path.isfile(feats) or not os.access(feats, os.R_OK):
        raise FileNotFoundError("--image %s: no readable features.pt (pre-extracted region features, see dataset.RegionFeatures)"
                                % options.image_dir)
    if not options.train_path:
        raise ValueError("--image needs the caption file (--train)")
    return dataset.ImageCaptionDataset(root_img_dir=options.image_dir, data_bin_file=options.train_path,
                                       max_capacity=int(options.img_capacity), text_processor=tp,
                                       max_img_per_batch=int(options.max_image), use_neg_samples=options.mm_mode != "masked",
                                       neg_seed=options.seed, lex_dict=lex_dict)


def run_phases(trainer, options, step, mt_train, mass_train, mt_dev=None, img_train=None, lang_directions=None):
    """The two phases of ``train`` from ``step`` on -- a fresh run's 0, or where a loaded snapshot stands (``trainer.phase``,
    ``epoch``, ``epoch_pos``): --step ordinary steps, then --fstep back-translation steps.  Returns the step count."""
    optimizer = trainer.optimizer
    if trainer.phase == "train":
        trainer.phase_bound = options.step  # --step is a total: a resumed run stops where the uninterrupted one would
    while trainer.phase == "train" and step < options.step and trainer.epochs_begun - trainer.phase_epoch0 < options.num_epochs:
        step = trainer.train_epoch(mt_data=mt_train, mass_data=mass_train, dev_data=mt_dev, step=step, max_step=options.step,
                                   save_path=options.model_path, log_every=options.log_steps, eval_every=options.eval_steps,
                                   accum=options.accum, img_data=img_train)
    # back-translation phase (src/train_image_mt.py:509-533): optimizer schedule reset, then --fstep more steps in which the
    # monolingual batches are back-translated.  The reference's flag default is 125000 steps; here the phase runs only when a
    # language pair is given (--langs), which is what makes it well-defined.
    if lang_directions is not None and options.finetune_step > 0 and mass_train:
        if trainer.phase != "bt":  # (a run resumed inside this phase goes on with its schedule: no second reset)
            optimizer.reset()
            trainer.begin_phase("bt", step + options.finetune_step)
        total = trainer.phase_bound = trainer.phase_start_step + options.finetune_step
        while step < total and trainer.epochs_begun - trainer.phase_epoch0 < options.num_epochs:
            step = trainer.train_epoch(mt_data=None if options.ignore_mt_mass else mt_train, mass_data=mass_train, dev_data=mt_dev,
                                       step=step, max_step=total, save_path=options.model_path, log_every=options.log_steps,
                                       eval_every=options.eval_steps, accum=options.accum, fine_tune=True,
                                       lang_directions=lang_directions)
    return step


def train(options):
    reject_off_path(options, lm_supported=True, dict_supported=True)
    resume = resume_dir_of(options)  # --resume DIR: the model is built from DIR as --pretrained builds it
    if options.lm_path and (options.pretrained_path or resume):
        raise ValueError("--lm %s with %s: a model loaded from a directory already has its weights; --lm initialises a fresh "
                         "model from a masked language model" % (options.lm_path, "--resume" if resume else "--pretrained"))
    if getattr(options, "image_dir", "") and len([l for l in (options.bt_langs or "").split(",") if l.strip()]) >= 2 \
            and options.finetune_step > 0:
        raise NotImplementedError("--image with --langs / --fstep: back-translation over image batches (src/train_image_mt.py:108-198 "
                                  "with is_img_batch) is not built; give --fstep 0 or drop --langs")
    rank, world = init_distributed()
    random.seed(options.seed)
    torch.manual_seed(options.seed)
    tp = TextProcessor(options.tokenizer_path)
    lex_dict = load_lex_dict(options)  # once: every dataset and the back-translation phase share it
    img_train = load_image_data(options, tp, lex_dict)  # before the model is built: a missing features.pt fails at once
    if img_train is not None and world > 1:
        raise NotImplementedError("--image under data parallelism is not built (ImageMTTrainer.image_step)")
    if resume or options.pretrained_path:
        model = ImageMassSeq2Seq.load(ImageMassSeq2Seq, resume or options.pretrained_path, tok_dir=options.tokenizer_path)
    else:
        model = ImageMassSeq2Seq(text_processor=tp, lang_dec=options.lang_decoder, tie_embed=options.tie_embed,
                                 use_proposals=lex_dict is not None,
                                 enc_layer=options.encoder_layer, dec_layer=options.decoder_layer, embed_dim=options.embed_dim,
                                 intermediate_dim=options.intermediate_layer_dim, num_attention_heads=options.heads,
                                 resnet_depth=options.resnet_depth, image_feat_dim=options.feat_dim)
        if options.lm_path:  # (the reference builds a FRESH LM here and never reads the path, :449-452: DESIGN section 1)
            from .lm import LM
            model.init_from_lm(LM.load(options.lm_path))
    use_lex_dict(model, lex_dict, "train_image_mt")
    model.set_compute_dtype(torch.float32 if options.fp32 else torch.bfloat16)
    model = model.cuda().train()
    optimizer = build_optimizer(model, options.learning_rate, options.warmup)
    # (GradSync broadcasts rank 0's parameters, like the DDP constructor at src/train_image_mt.py:73)
    trainer = ImageMTTrainer(model, mask_prob=options.mask_prob, clip=options.clip, optimizer=optimizer, rank=rank, world_size=world,
                             seed=options.seed, bt_beam_width=options.bt_beam_width, max_len_a=options.max_len_a,
                             max_len_b=options.max_len_b, len_penalty_ratio=options.len_penalty_ratio, mm_mode=options.mm_mode,
                             lex_dict=lex_dict, bt_sampling=getattr(options, "bt_sampling", False),
                             bt_topk=getattr(options, "bt_topk", 0), bt_temperature=getattr(options, "bt_temperature", 1.0))
    pad = tp.pad_token_id()
    kw = dict(max_batch_capacity=options.total_capacity, max_batch=options.batch, pad_idx=pad, max_seq_len=options.max_seq_len,
              ngpu=1, lex_dict=lex_dict)
    mt_train = batches_from(options.mt_train_path, **kw)
    mass_train = batches_from(options.mass_train_path, dataset.MassDataset, **kw)
    mt_dev = batches_from(options.mt_dev_path, **kw) or None
    if rank == 0:
        print("MT batches", len(mt_train), "MASS batches", len(mass_train), "image batches", len(img_train or []),
              "dev batches", len(mt_dev or []), flush=True)
    step = trainer.begin_run(options, resume)
    step = run_phases(trainer, options, step, mt_train, mass_train, mt_dev, img_train, ImageMTTrainer.get_lang_dirs(options.bt_langs, tp))
    trainer.finish_snapshots()  # (before the closing evaluation: a resumed run meets best_loss as the loop left it)
    if mt_dev is not None:
        trainer.validate_and_save(mt_dev, options.model_path)
    elif rank == 0 and options.model_path:
        model.save(options.model_path)
    return trainer


def main(argv=None):
    options, _ = get_option_parser().parse_args(argv)
    train(options)


if __name__ == "__main__":
    main()
