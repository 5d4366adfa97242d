"""CPU suite: weighted and long prompts on the host (vdx/prompt.py, vdx/options.py): the parser on the web UI's published examples
and against the independent restatement of tests/prompt_ref.py; the chunker with the hash tokenizer at every edge of a chunk, with
commas, `BREAK`, the empty text and the cap; the option, its refusals and its record; the ctypes row of the new entry point."""
import os
import random
import sys

import pytest
import torch

import vdx  # noqa: F401
from vdx import _lib
from vdx.compat.diffusers_shim import HashTokenizer
from vdx.prompt import BREAK, chunk_tokens, parse_attention, plan_texts, strip_syntax

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prompt_ref as R  # noqa: E402

TOK = HashTokenizer()
BOS, EOS = TOK.bos_token_id, TOK.eos_token_id


def ids_of(text):
    return TOK(text, add_special_tokens=False, truncation=False, padding=False, return_tensors=None).input_ids


COMMA = ids_of(",")[0]


def words(n, start=0):
    return [f"w{start + j}" for j in range(n)]


def chunked(text, max_chunks=4):
    return chunk_tokens(parse_attention(text), TOK, max_chunks)


def inner(ids):
    """Per chunk, the tokens between BOS and the first EOS."""
    return [row[1:1 + row[1:].tolist().index(EOS)].tolist() for row in ids]


# ---- the parser ---------------------------------------------------------------------------------------------------------------
def test_parser_on_the_published_examples():
    assert parse_attention("an (important) word") == [("an ", 1.0), ("important", 1.1), (" word", 1.0)]
    assert parse_attention("(unbalanced") == [("unbalanced", 1.1)]
    assert parse_attention("\\(literal\\]") == [("(literal]", 1.0)]
    assert parse_attention("(unnecessary)(parens)") == [("unnecessaryparens", 1.1)]
    assert parse_attention("normal text") == [("normal text", 1.0)]
    assert parse_attention("") == [("", 1.0)]


def test_parser_on_the_nested_example_weights_are_the_products_in_order():
    """Every weight is compared with the product formed the way the parser forms it (innermost closer first, the opener left open
    closed at the end), not with a decimal literal.  `sky` stands inside three closed pairs and the one left open: 1.1^4
    (1.4641000000000006 in the web UI's own docstring), as ' ', ' a ', ', sun, ' and '.' inside the same open bracket carry 1.1."""
    got = parse_attention("a (((house:1.3)) [on] a (hill:0.5), sun, (((sky))).")
    want = [("a ", 1.0), ("house", 1.0 * 1.3 * 1.1 * 1.1), (" ", 1.0 * 1.1), ("on", 1.0 * (1 / 1.1) * 1.1), (" a ", 1.0 * 1.1),
            ("hill", 1.0 * 0.5 * 1.1), (", sun, ", 1.0 * 1.1), ("sky", 1.0 * 1.1 * 1.1 * 1.1 * 1.1), (".", 1.0 * 1.1)]
    assert got == want
    assert got[3][1] == 1.0 and got[5][1] == 0.55


def test_parser_escapes_break_and_stray_closers():
    assert parse_attention("a \\\\ b") == [("a \\ b", 1.0)]
    assert parse_attention("a) b] c") == [("a) b] c", 1.0)]
    assert parse_attention("a:1.5) b") == [("a:1.5) b", 1.0)]                       # nothing open: text
    assert parse_attention("[a]") == [("a", 1 / 1.1)]
    assert parse_attention("(a:1.5) b BREAK (c)") == [("a", 1.5), (" b", 1.0), BREAK, ("", 1.0), ("c", 1.1)]
    assert parse_attention("aBREAK b") == [("aBREAK b", 1.0)]                       # not a word of its own
    assert strip_syntax("a (red coat:1.3) BREAK [dull] \\(sic\\)") == "a red coat dull (sic)"
    with pytest.raises(ValueError, match="string"):
        parse_attention(None)


def test_parser_equals_the_restatement_on_seeded_soup():
    rnd = random.Random(7)
    alphabet = ["a", "b", " ", " , ", "(", ")", "[", "]", ":1.2)", ":", ": 0.5 )", "\\(", "\\", "\\\\", " BREAK ", "BREAK", "xBREAK", ":1.2.3)", ":-2)"]
    for _ in range(2000):
        text = "".join(rnd.choice(alphabet) for _ in range(rnd.randint(0, 14)))
        assert parse_attention(text) == R.parse(text), text


# ---- the chunker --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lengths", [(74, [74]), (75, [75]), (76, [75, 1]), (150, [75, 75]), (151, [75, 75, 1])])
def test_chunker_at_the_edges_of_a_chunk(n, lengths):
    ws = words(n)
    ids, wts = chunked(" ".join(ws))
    assert ids.dtype == torch.int64 and wts.dtype == torch.float32 and tuple(ids.shape) == tuple(wts.shape) == (len(lengths), 77)
    assert [len(c) for c in inner(ids)] == lengths
    assert [t for c in inner(ids) for t in c] == [ids_of(w)[0] for w in ws]        # every token, in order, none dropped
    assert bool((ids[:, 0] == BOS).all()) and bool((wts == 1.0).all())
    for row, k in zip(ids, lengths):
        assert bool((row[1 + k:] == EOS).all())


def test_chunker_splits_behind_a_comma_in_the_last_twenty():
    """80 tokens, a comma as token 60 (0-based): chunk 0 ends with the comma (61 tokens), the 14 behind it open chunk 1."""
    ws = words(60) + [","] + words(19, 100)
    ids, _ = chunked(" ".join(ws))
    a, b = inner(ids)
    assert len(a) == 61 and a[-1] == COMMA and b == [ids_of(w)[0] for w in ws[61:]]
    # the comma as the chunk's very first candidate (token 55) and as its last token (74: an ordinary split)
    assert [len(c) for c in inner(chunked(" ".join(words(55) + [","] + words(24, 100)))[0])] == [56, 24]
    assert [len(c) for c in inner(chunked(" ".join(words(74) + [","] + words(5, 100)))[0])] == [75, 5]
    # token 75 is itself a comma: the chunk is full and splits at 75
    assert [len(c) for c in inner(chunked(" ".join(words(60) + [","] + words(14, 100) + [","] + words(4, 200)))[0])] == [75, 5]


def test_chunker_ignores_a_comma_further_back():
    ws = words(54) + [","] + words(25, 100)                                      # token 54: 21 back from the end of the chunk
    assert [len(c) for c in inner(chunked(" ".join(ws))[0])] == [75, 5]


def test_break_pads_out_the_chunk_and_weights_follow_their_tokens():
    ids, wts = chunked("a (b c:1.3) BREAK [d] e")
    assert [len(c) for c in inner(ids)] == [3, 2]
    assert wts[0, :5].tolist() == [1.0, 1.0, torch.tensor(1.3).item(), torch.tensor(1.3).item(), 1.0]
    assert wts[1, :4].tolist() == [1.0, torch.tensor(1 / 1.1).item(), 1.0, 1.0]
    assert bool((wts[0, 4:] == 1.0).all()) and bool((wts[1, 3:] == 1.0).all())   # EOS and padding
    assert bool((ids[0, 4:] == EOS).all())
    assert [len(c) for c in inner(chunked("a BREAK")[0])] == [1]
    assert [len(c) for c in inner(chunked("BREAK a")[0])] == [0, 1]


def test_the_empty_text_is_one_chunk_and_equals_the_plain_call():
    ids, wts = chunked("")
    assert tuple(ids.shape) == (1, 77) and ids[0, 0] == BOS and bool((ids[0, 1:] == EOS).all()) and bool((wts == 1.0).all())
    for text in ("", "a rocket in space, 4k", " ".join(words(75))):
        plain = TOK([text], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        assert torch.equal(chunked(text)[0], plain)


def test_the_cap_is_refused_and_names_the_count():
    assert tuple(chunked(" ".join(words(300)))[0].shape) == (4, 77)
    with pytest.raises(ValueError, match=r"301 tokens.*5 chunks"):
        chunked(" ".join(words(301)))
    with pytest.raises(ValueError, match="76 tokens"):
        chunked(" ".join(words(76)), max_chunks=1)


def test_chunker_equals_the_restatement_on_seeded_streams():
    rnd = random.Random(3)
    for _ in range(150):
        text = " ".join(rnd.choice([f"w{rnd.randint(0, 50)}", ",", "(", ")", "BREAK"]) for _ in range(rnd.randint(0, 280)))
        ids, wts = chunked(text, max_chunks=99)
        rid, rw, _ = R.chunks(R.parse(text), ids_of, BOS, EOS, EOS, COMMA)
        assert torch.equal(ids, rid) and torch.equal(wts, rw), text


def test_plan_pads_every_text_to_the_largest_chunk_count():
    plan = plan_texts([" ".join(words(100)), "", "a (b:1.2)"], TOK)
    assert tuple(plan.ids.shape) == (3, 2, 77) and plan.tokens == (100, 0, 2) and plan.chunks == 2 and plan.weighted
    empty = chunked("")[0][0]
    assert torch.equal(plan.ids[1, 0], empty) and torch.equal(plan.ids[1, 1], empty) and torch.equal(plan.ids[2, 1], empty)
    assert plan.record() == {"syntax": "a1111", "chunks": 2, "tokens": [100, 0, 2], "weighted": True}
    assert not plan_texts(["a b", ""], TOK).weighted


def test_hash_tokenizer_keeps_its_present_outputs():
    ids = TOK(["a rocket in space", ""], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert tuple(ids.shape) == (2, 77) and ids[0, 0] == BOS and ids[0, 5] == EOS and bool((ids[1, 1:] == EOS).all())
    assert ids[0, 1:5].tolist() == ids_of("a rocket in space")
    long = TOK(" ".join(words(100)), return_tensors="pt").input_ids
    assert tuple(long.shape) == (1, 77) and long[0, -1] == EOS and long[0, 1:76].tolist() == [ids_of(w)[0] for w in words(75)]
    assert len(ids_of(" ".join(words(100)))) == 100 and ids_of("") == []


# ---- the option ---------------------------------------------------------------------------------------------------------------
def test_option_default_refusals_and_record():
    from vdx.options import RECORD_KEYS, JobOptions, check_prompt_syntax, prompt_record, resolve
    from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args
    assert DiffuserConfig().prompt_syntax == "plain" and build_arg_parser().parse_args([]).prompt_syntax == "plain"
    off = resolve(DiffuserConfig(), job=True)
    assert off.prompt_syntax == "plain" and prompt_record(off) == {} and "prompt_syntax" not in RECORD_KEYS
    cfg = config_from_args(build_arg_parser().parse_args(["--prompt_syntax", "a1111", "--prompt", "a (fox:1.2)"]))
    on = resolve(cfg, job=True)
    assert isinstance(on, JobOptions) and on.prompt_syntax == "a1111" and resolve(cfg).prompt_syntax == "a1111"
    assert prompt_record(on) == {}                                               # no record before the texts are encoded
    with pytest.raises(ValueError, match="prompt_syntax must be one of"):
        resolve(DiffuserConfig(prompt_syntax="compel"), job=True)
    with pytest.raises(ValueError, match="prompt_syntax must be one of"):
        resolve(DiffuserConfig(prompt_syntax="compel"))
    long = " ".join(words(301))
    for kw in (dict(prompt=long), dict(negative_prompt=long), dict(prompt_travel=((3, long),))):
        with pytest.raises(ValueError, match="301 tokens"):
            resolve(DiffuserConfig(prompt_syntax="a1111", num_frames=8, **kw), job=True)
    assert resolve(DiffuserConfig(prompt=long), job=True).prompt_syntax == "plain"     # "plain" truncates, as always
    assert check_prompt_syntax(DiffuserConfig(prompt_syntax="a1111", prompt=long)) == "a1111"   # a call brings its own embeddings
    import dataclasses
    rec = plan_texts(["a (fox:1.2)", ""], TOK).record()
    found = dataclasses.replace(on, prompt_found=rec)
    assert prompt_record(found) == {"prompt_syntax": rec} and set(rec) == {"syntax", "chunks", "tokens", "weighted"}
    assert prompt_record({"prompt_syntax": rec, "x": 1}) == {"prompt_syntax": rec} and prompt_record({"x": 1}) == {}


def test_unet_text_padding_rule():
    from vdx.unet3d import MAX_TEXT_LEN, TEXT_PAD, text_pad_of
    assert TEXT_PAD == 128 and MAX_TEXT_LEN == 308
    assert [text_pad_of(n) for n in (1, 77, 128, 129, 154, 192, 193, 231, 308)] == [128, 128, 128, 192, 192, 192, 256, 256, 320]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_ctypes_row_of_the_new_entry_matches_the_header():
    from test_host import _abi_mismatches, _header_declarations
    decls = _header_declarations()
    name = "vdx_prompt_weight_f16"
    assert name in decls and name in _lib.SIGNATURES
    ret, params = decls[name]
    assert ret == "int" and len(params) == 7 == len(_lib.SIGNATURES[name][1])
    assert _abi_mismatches({name: _lib.SIGNATURES[name]}, {name: decls[name]}) == []
    import ctypes
    res, args = _lib.SIGNATURES[name]
    assert _abi_mismatches({name: (res, args[:3] + [ctypes.c_size_t] + args[4:])}, {name: decls[name]}) == [name]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
