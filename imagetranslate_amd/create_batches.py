"""Tokenise a text file into the marshal blocks ``TextDataset`` reads -- counterpart of src/create_batches.py (same files:
``<cache_dir>/N.pkl`` = marshal of {row number: (ids, language index)} with ``sen_block_size`` rows per block, and ``info.txt`` =
block size TAB rows TAB files).  Every non-empty line is a document: ``TextProcessor.tokenize_lines(blind_split=True)`` cuts it
into rows of ``seq_len`` ids; the language of its rows is that of the line's first id, which must be a language tag.

As in the reference a last block is written after the full ones even when it is empty (the rows fill their blocks exactly), and
nothing but ``info.txt`` for a file without documents.  The reference tokenises in chunks of 100 000 rows and loses the open
block when the file ends exactly on a chunk; here rows go to their blocks as they come, so that cannot happen."""
import marshal
import os
from optparse import OptionParser

from .textprocessor import TextProcessor


def write(text_processor: TextProcessor, cache_dir: str, seq_len: int, txt_file: str, sen_block_size: int = 10000):
    """Returns (rows, files)."""
    examples, line_num, file_count, documents = {}, 0, 0, 0
    text_processor.max_len = seq_len

    def flush():
        nonlocal examples, file_count
        with open(os.path.join(cache_dir, str(file_count) + ".pkl"), "wb") as fw:
            marshal.dump(examples, fw)
        examples, file_count = {}, file_count + 1

    with open(txt_file, "r") as fp:
        for line in fp:
            line = line.strip()
            if not line:
                continue
            documents += 1
            rows = text_processor.tokenize_lines(line, blind_split=True, split_len=seq_len)
            lang = text_processor.languages[text_processor.id2token(int(rows[0, 0]))]
            for row in rows:
                examples[line_num] = (row.tolist(), lang)
                line_num += 1
                if len(examples) >= sen_block_size:
                    flush()
    if documents:
        flush()
        print("from %d documents, dumped %d vectors into %d files" % (documents, line_num, file_count))
    with open(os.path.join(cache_dir, "info.txt"), "w") as fw:
        fw.write(str(sen_block_size) + "\t" + str(line_num) + "\t" + str(file_count))
    return line_num, file_count


def get_tokenizer(tokenizer_path: str = None, train_path: str = None, model_path: str = None, vocab_size: int = None) -> TextProcessor:
    """The tokenizer of ``tokenizer_path``, or one trained on ``train_path`` and saved to ``model_path`` (src/create_batches.py:
    56-88): the training text is the file's sentences (split at ``</s>``) without the leading language tags, which become the
    tokenizer's languages in sorted order.  The tokenizer's files are written with ``save_model``, as everywhere in this project."""
    if tokenizer_path is not None:
        return TextProcessor(tokenizer_path)
    if not model_path or not train_path or not vocab_size:
        raise ValueError("without --tok a tokenizer is trained: --data (the text), --model (where it is saved) and --vocab_size "
                         "are required")
    os.makedirs(model_path, exist_ok=True)
    languages, tmp = set(), train_path + ".tmp"
    with open(tmp, "w") as wf, open(train_path, "r") as rf:
        for line in rf:
            sens = [sen.strip() for sen in line.split("</s>") if len(sen.strip()) > 0]
            if not sens:
                continue
            if sens[0].startswith("<"):
                words = sens[0].split(" ")
                languages.add(words[0])
                sens[0] = " ".join(words[1:])
            wf.write("\n".join(sens) + "\n")
    text_processor = TextProcessor()
    try:
        text_processor.train_tokenizer(paths=[tmp], vocab_size=vocab_size, to_save_dir=model_path,
                                       languages={l: i for i, l in enumerate(sorted(languages))})
    finally:
        os.remove(tmp)
    return text_processor


def main(argv=None):
    parser = OptionParser()
    parser.add_option("--data", dest="data_path", help="text file: one document per line", metavar="FILE", default=None)
    parser.add_option("--cache", dest="cache_path", help="directory for the marshal blocks", metavar="FILE", default=None)
    parser.add_option("--tok", dest="tokenizer_path", help="tokenizer directory (trained on --data into --model without it)",
                      metavar="FILE", default=None)
    parser.add_option("--block", dest="sentence_block", help="rows per block", type="int", default=10000)
    parser.add_option("--len", dest="seq_len", help="row length", type="int", default=512)
    parser.add_option("--vocab_size", dest="vocab_size", type="int", default=30000)
    parser.add_option("--model", dest="model_path", help="where a newly trained tokenizer is saved", metavar="FILE", default=None)
    options, _ = parser.parse_args(argv)
    if not options.data_path or not options.cache_path:
        parser.error("--data and --cache are required")
    tp = get_tokenizer(tokenizer_path=options.tokenizer_path, train_path=options.data_path, model_path=options.model_path,
                       vocab_size=options.vocab_size)
    os.makedirs(options.cache_path, exist_ok=True)
    write(text_processor=tp, cache_dir=options.cache_path, seq_len=options.seq_len, txt_file=options.data_path,
          sen_block_size=options.sentence_block)
    print("finished")


if __name__ == "__main__":
    main()
