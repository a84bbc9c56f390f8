"""Reading the reference's pickled side files -- ``mt_config`` (a 9-tuple of bool/int, src/seq2seq.py:183-196; a 3-tuple of
int for Caption2Image, src/image_model.py:445-446) and the tokenizer directory's ``langs`` (Dict[str, int], src/textprocessor.py:42-45) -- without executing anything from the
file: an Unpickler whose ``find_class`` always refuses.  Builtin containers and scalars need no class lookup, so the
reference's files load unchanged; a pickle that names any global (the vehicle of pickle code execution) is rejected.
"""
import io
import pickle


class _NoGlobals(pickle.Unpickler):
    def find_class(self, module, name):
        raise pickle.UnpicklingError("refusing to resolve %s.%s: only plain containers and scalars are accepted" % (module, name))


def load_plain(fp):
    data = fp.read() if hasattr(fp, "read") else fp
    return _NoGlobals(io.BytesIO(data)).load()


def load_mt_config(path):
    """(lang_dec, use_proposals, enc_layer, dec_layer, embed_dim, intermediate_dim, tie_embed, resnet_depth, freeze_image)"""
    with open(path, "rb") as fp:
        cfg = load_plain(fp)
    if not isinstance(cfg, tuple) or len(cfg) != 9 or not all(isinstance(v, (bool, int)) for v in cfg):
        raise ValueError("%s: expected the reference's 9-tuple of bool/int, got %r" % (path, type(cfg)))
    return cfg


def load_caption2image_config(path):
    """(enc_layer, embed_dim, intermediate_dim) of a Caption2Image directory (src/image_model.py:445-446)"""
    with open(path, "rb") as fp:
        cfg = load_plain(fp)
    if not isinstance(cfg, tuple) or len(cfg) != 3 or not all(isinstance(v, int) and not isinstance(v, bool) for v in cfg):
        raise ValueError("%s: expected the reference's 3-tuple of int, got %r" % (path, type(cfg)))
    return cfg


_CONFIG_TYPES = (bool, int, float, str, type(None))


def _check_lm_config(cfg, what):
    if not isinstance(cfg, dict):
        raise ValueError("%s: expected a dict of config fields, got %r" % (what, type(cfg)))
    for k, v in cfg.items():
        if not isinstance(k, str) or not isinstance(v, _CONFIG_TYPES):
            raise ValueError("%s: config field %r holds %r; only bool / int / float / str / None values can be written and read "
                             "back without executing anything" % (what, k, type(v)))
    return cfg


def save_lm_config(cfg: dict, path):
    """Write the config fields of an LM as a pickled plain dict -- what ``load_lm_config`` reads.  A field whose value is not a
    scalar is an error, not something to leave out: the file must give back the config it was written from."""
    with open(path, "wb") as fp:
        pickle.dump(dict(_check_lm_config(cfg, path)), fp)


def load_lm_config(path):
    """The ``config`` file of an LM directory as a plain dict of config fields.  ``lm.LM.save`` writes a dict; the reference pickles
    a ``transformers.BertConfig`` instance (src/lm.py:60-61), which cannot be read without importing and running what the file
    names -- such a file is refused."""
    with open(path, "rb") as fp:
        try:
            cfg = load_plain(fp)
        except pickle.UnpicklingError as err:
            raise ValueError("%s holds a pickled object, not a plain dict of config fields (%s); a config pickled as a class "
                             "instance would have to be executed to be read -- save the fields as a dict "
                             "(pickle.dump(config.to_dict(), fp))" % (path, err)) from None
    return _check_lm_config(cfg, path)


def load_langs(path):
    with open(path, "rb") as fp:
        langs = load_plain(fp)
    if not isinstance(langs, dict) or not all(isinstance(k, str) and isinstance(v, int) and not isinstance(v, bool)
                                              for k, v in langs.items()):
        raise ValueError("%s: expected Dict[str, int] of language tags" % path)
    return langs
