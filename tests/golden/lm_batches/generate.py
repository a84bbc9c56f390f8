"""Regenerates this fixture: python generate.py /path/to/reference/src

  tok/            a 1000-token SentencePiece-BPE tokenizer (vocab.json, merges.txt, langs) trained by this project's
                  TextProcessor.train_tokenizer on tests/golden/sample_enfa
  lines.txt       30 documents: '<en>' / '<fa>' + three consecutive sentences of sample_enfa joined by ' </s> ', and two blank lines
  cache/          what the REFERENCE's create_batches.write(text_processor, cache, seq_len=SEQ_LEN, lines.txt, sen_block_size=BLOCK)
                  wrote from them with the reference's TextProcessor on tok/: the marshal blocks N.pkl and info.txt
  meta.json       SEQ_LEN, BLOCK and the counts

The reference's code runs in a child process that imports it from the given directory; nothing of it is copied here.  Tests read
the recorded files only (tests/test_lm_host.py) and never import this script."""
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
SEQ_LEN, BLOCK, DOCS = 32, 10, 30

CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import create_batches
from textprocessor import TextProcessor
create_batches.write(text_processor=TextProcessor(sys.argv[2]), cache_dir=sys.argv[3], seq_len=int(sys.argv[4]), txt_file=sys.argv[5],
                     sen_block_size=int(sys.argv[6]))
"""


def main(reference_src):
    sys.path.insert(0, ROOT)
    from imagetranslate_amd.textprocessor import TextProcessor
    sample = os.path.join(ROOT, "tests", "golden", "sample_enfa")
    tok, cache = os.path.join(HERE, "tok"), os.path.join(HERE, "cache")
    for d in (tok, cache):
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
    TextProcessor().train_tokenizer([os.path.join(sample, "en.txt"), os.path.join(sample, "fa.txt")], vocab_size=1000, to_save_dir=tok,
                                    languages={"<en>": 0, "<fa>": 1})
    os.remove(os.path.join(tok, "tokenizer.json"))  # vocab.json + merges.txt: the layout the reference reads
    text = {l: [s for s in open(os.path.join(sample, l + ".txt"), encoding="utf-8").read().split("\n") if s.strip()] for l in ("en", "fa")}
    lines = []
    for i in range(DOCS):
        lang = "en" if i % 2 == 0 else "fa"
        lines.append("<%s> %s" % (lang, " </s> ".join(text[lang][3 * i:3 * i + 3])))
        if i in (4, 17):
            lines.append("")
    txt = os.path.join(HERE, "lines.txt")
    with open(txt, "w", encoding="utf-8") as fw:
        fw.write("\n".join(lines) + "\n")
    subprocess.run([sys.executable, "-c", CHILD, reference_src, tok, cache, str(SEQ_LEN), txt, str(BLOCK)], check=True)
    block, rows, files = open(os.path.join(cache, "info.txt")).read().strip().split("\t")
    with open(os.path.join(HERE, "meta.json"), "w") as fw:
        json.dump({"source": "rasoolims/ImageTranslate src/create_batches.py write(), src/textprocessor.py tokenize_lines()",
                   "seq_len": SEQ_LEN, "block": int(block), "rows": int(rows), "files": int(files), "documents": DOCS}, fw, indent=1)
        fw.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
