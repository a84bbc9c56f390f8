"""Sentence-pair scoring -- counterpart of src/get_sen_sim.py (``SenSimEval.eval`` ``:18-52``, ``sim`` ``:54-71``): a saved
``SenSim`` scores every pair of ``--dev_mt`` (``forward(normalize=False)``: encoder stack, fused pooling, ``imt_pair_dot``) and
``--output`` receives one ``source \\t target \\t similarity`` line per pair, the texts decoded until ``</s>`` with the first
token (the language tag) removed."""
import torch

from . import dataset
from .option_parser import get_img_options_parser
from .sen_sim import SenSim
from .seq_gen import get_outputs_until_eos


@torch.no_grad()
def score_batch(model, batch):
    """(source texts, target texts, similarities as floats) of one MT batch."""
    tp = model.text_processor
    sims = model(batch["src_texts"], batch["src_pad_mask"], batch["src_langs"], batch["dst_texts"], batch["dst_pad_mask"],
                 batch["dst_langs"], normalize=False).cpu()
    decode = lambda texts: [tp.tokenizer.decode(t.numpy()) for t in
                            get_outputs_until_eos(tp.sep_token_id(), texts, remove_first_token=True)]
    return decode(batch["src_texts"]), decode(batch["dst_texts"]), [float(s) for s in sims]


def sim(options):
    if not options.model_path or not options.mt_dev_path or not options.output:
        raise ValueError("--model, --dev_mt and --output are required")
    model, tp = SenSim.load(options.model_path, tok_dir=options.tokenizer_path)
    model = model.set_compute_dtype(torch.float32 if options.fp32 else torch.bfloat16).eval()
    data = dataset.MTDataset(batch_pickle_dir=options.mt_dev_path, max_batch_capacity=options.total_capacity,
                             max_batch=int(options.batch / (options.beam_width * 2)), pad_idx=tp.pad_token_id(),
                             keep_pad_idx=False)
    pairs = 0
    with open(options.output, "w") as w:
        for i in range(len(data)):
            srcs, tgts, sims = score_batch(model, data[i])
            for s, t, v in zip(srcs, tgts, sims):
                w.write(s + "\t" + t + "\t" + str(v) + "\n")
            pairs += len(sims)
            print(i + 1, "/", len(data), end="\r")
    print("\n")
    return pairs


def main(argv=None):
    options, _ = get_img_options_parser().parse_args(argv)
    sim(options)
    print("Finished!")


if __name__ == "__main__":
    main()
