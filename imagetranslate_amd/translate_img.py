"""Translate through predicted image embeddings -- counterpart of src/translate_img.py (flags ``:16-34``, ``translate_batch``
``:37-95``, output ``:140-163``): ``Caption2Image`` maps a sentence to the 49 x d region embedding of "its" image and a trained
``ImageCaptioning`` model decodes that embedding in the other language (beam search with ``image_embed=``).  Three hops per
sentence: source -> target, that output back to the source language, and that output to the target language again; every hop
re-embeds the previous hop's output."""
import datetime
from optparse import OptionParser

import torch
import torch.utils.data as data_utils
from torch.nn.utils.rnn import pad_sequence

from . import dataset
from .image_model import Caption2Image, ImageCaptioning
from .seq2seq import Seq2Seq
from .seq_gen import BeamDecoder, get_outputs_until_eos

REGIONS = Caption2Image.REGIONS


def get_lm_option_parser():
    parser = OptionParser()
    parser.add_option("--input", dest="input_path", metavar="FILE", default=None)
    parser.add_option("--src", dest="src_lang", type="str", default=None)
    parser.add_option("--target", dest="target_lang", type="str", default=None)
    parser.add_option("--output", dest="output_path", metavar="FILE", default=None)
    parser.add_option("--batch", dest="batch", help="Batch size", type="int", default=512)
    parser.add_option("--tok", dest="tokenizer_path", help="Path to the tokenizer folder", metavar="FILE", default=None)
    parser.add_option("--cache_size", dest="cache_size", help="Number of blocks in cache", type="int", default=300)
    parser.add_option("--model", dest="model_path", metavar="FILE", default=None)
    parser.add_option("--caption-model", dest="caption_model_path", metavar="FILE", default=None)
    parser.add_option("--verbose", action="store_true", dest="verbose", help="Include input!", default=False)
    parser.add_option("--beam", dest="beam_width", type="int", default=4)
    parser.add_option("--max_len_a", dest="max_len_a", help="a for beam search (a*l+b)", type="float", default=1.3)
    parser.add_option("--max_len_b", dest="max_len_b", help="b for beam search (a*l+b)", type="int", default=5)
    parser.add_option("--len-penalty", dest="len_penalty_ratio", help="Length penalty", type="float", default=0.8)
    parser.add_option("--capacity", dest="total_capacity", help="Batch capacity", type="int", default=150)
    parser.add_option("--fp16", action="store_true", dest="fp16", default=False)
    parser.add_option("--fp32", action="store_true", dest="fp32", default=False)  # build addition: compute in fp32 (default bf16)
    return parser


def _decode_all(text_processor, outputs):
    return [text_processor.tokenizer.decode(o[1:].tolist()) for o in outputs]


@torch.no_grad()
def translate_batch(batch, txt2img, generator, text_processor, verbose=False):
    """(hop-1 texts, source texts or None, hop-2 texts, hop-3 texts) of one MTDataset batch (src/translate_img.py:37-95)."""
    pad_idx = text_processor.pad_token_id()
    src_inputs = batch["src_texts"].squeeze(0)
    src_mask = batch["src_pad_mask"].squeeze(0)
    tgt_inputs = batch["dst_texts"].squeeze(0)
    src_langs = batch["src_langs"].squeeze(0)
    dst_langs = batch["dst_langs"].squeeze(0)
    src_text = None
    if verbose:
        src_ids = get_outputs_until_eos(text_processor.sep_token_id(), src_inputs, remove_first_token=True)
        src_text = [text_processor.tokenizer.decode(s.tolist()) for s in src_ids]
    gen_module = generator.module if hasattr(generator, "module") else generator
    max_len = min(int(gen_module.max_len_a * src_inputs.size(1) + gen_module.max_len_b), 512)

    def hop(inputs, mask, in_langs, first_tokens, out_langs):
        image_embed = txt2img(inputs, mask, in_langs)
        image_embed = image_embed.view(image_embed.size(0), REGIONS, -1)
        outputs = generator(first_tokens=first_tokens, max_len=max_len, tgt_langs=out_langs, image_embed=image_embed,
                            pad_idx=pad_idx)
        outputs = [o.cpu() for o in outputs]
        padded = pad_sequence(outputs, batch_first=True, padding_value=pad_idx)
        return outputs, padded, padded != pad_idx

    outputs, padded, mask = hop(src_inputs, src_mask, src_langs, tgt_inputs[:, 0], dst_langs)
    second, padded2, mask2 = hop(padded, mask, dst_langs, src_inputs[:, 0], src_langs)
    third, _, _ = hop(padded2, mask2, src_langs, tgt_inputs[:, 0], dst_langs)
    return _decode_all(text_processor, outputs), src_text, _decode_all(text_processor, second), _decode_all(text_processor, third)


def format_outputs(mt_output, src_text, mt_2nd_output, mt_3rd_output, verbose=False):
    """What one batch adds to the output file (src/translate_img.py:155-161): a hop-1 line per sentence, or, verbose, the
    five-line block source / hop 1 / hop 2 / hop 3 / ****."""
    if not verbose:
        return "\n".join(mt_output) + "\n"
    return "\n".join(y + "\n" + x + "\n" + z + "\n" + f + "\n****"
                     for x, y, z, f in zip(mt_output, src_text, mt_2nd_output, mt_3rd_output)) + "\n"


def build_data_loader(options, text_processor):
    assert options.src_lang is not None and options.target_lang is not None
    src_lang = "<" + options.src_lang + ">"
    dst_lang = "<" + options.target_lang + ">"
    src_lang_id, target_lang = text_processor.languages[src_lang], text_processor.languages[dst_lang]
    fixed_output = [text_processor.token_id(dst_lang)]
    examples = []
    with open(options.input_path, "r") as s_fp:
        for src_line in s_fp:
            if len(src_line.strip()) == 0:
                continue
            src_line = " ".join([src_lang, src_line, "</s>"])
            src_tok_line = text_processor.tokenize_one_sentence(src_line.strip().replace(" </s> ", " "))
            examples.append((src_tok_line, fixed_output, src_lang_id, target_lang))
    test_data = dataset.MTDataset(examples=examples, max_batch_capacity=options.total_capacity, max_batch=options.batch,
                                  pad_idx=text_processor.pad_token_id(), max_seq_len=10000)
    return data_utils.DataLoader(test_data, batch_size=1, shuffle=False)


def build_model(options):
    dtype = torch.float32 if options.fp32 else torch.bfloat16
    model = Caption2Image.load(options.model_path, options.tokenizer_path).set_compute_dtype(dtype).cuda().eval()
    caption_model = Seq2Seq.load(ImageCaptioning, options.caption_model_path, tok_dir=options.tokenizer_path)
    caption_model = caption_model.set_compute_dtype(dtype).cuda().eval()
    generator = BeamDecoder(caption_model, beam_width=options.beam_width, max_len_a=options.max_len_a,
                            max_len_b=options.max_len_b, len_penalty_ratio=options.len_penalty_ratio)
    return model, generator, model.text_processor


def main(argv=None):
    options, _ = get_lm_option_parser().parse_args(argv)
    txt2img_model, generator, text_processor = build_model(options)
    test_loader = build_data_loader(options, text_processor)
    sen_count = 0
    with open(options.output_path, "w") as writer:
        for batch in test_loader:
            outs = translate_batch(batch, txt2img_model, generator, text_processor, options.verbose)
            sen_count += len(outs[0])
            writer.write(format_outputs(*outs, verbose=options.verbose))
    print(datetime.datetime.now(), "Translated", sen_count, "sentences")


if __name__ == "__main__":
    main()
