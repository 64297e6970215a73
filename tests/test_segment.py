"""rwkvtts.segment.split_text: its invariants over generated Chinese, English and mixed texts with
the project's tokenizer and with a one-token-per-character encoder, and a table of fixed examples."""
import os
import random

import pytest

from rwkvtts.segment import CUTS, Pauses, Segment, split_text
from rwkvtts.tokenizer import Tokenizer

HERE = os.path.dirname(os.path.abspath(__file__))
VOCAB = os.path.join(HERE, "..", "rwkv-tts-rs_amd", "assets", "tokenizer.json")


@pytest.fixture(scope="module")
def tok():
    return Tokenizer(VOCAB)


def chars(t):
    """One token per character."""
    return [ord(c) for c in t]


EN = ["The quick brown fox jumps over the lazy dog", "Speech synthesis, as it turns out, is hard", "Is it", "No",
      "Dr. Smith paid 3,000 dollars at 12:30", "Wait", "a" * 90, "She said \"go.\"", "Then (quietly) she left"]
ZH = ["今天天气很好", "我们去公园散步，然后回家吃饭", "你好吗", "这是一个没有任何标点符号的非常非常非常非常非常非常非常非常长的句子" * 3,
      "他说：“明天见。”", "好的", "第一、第二、第三"]
ENDS_EN, ENDS_ZH = [". ", "! ", "? ", "... ", ".\n", ".\n\n", "; ", ", ", " "], ["。", "！", "？", "……", "。\n", "；", "，"]


def generated(seed):
    rng = random.Random(seed)
    kind = seed % 3
    parts = []
    for _ in range(rng.randint(1, 14)):
        zh = kind == 1 or (kind == 2 and rng.random() < 0.5)
        parts.append(rng.choice(ZH if zh else EN) + rng.choice(ENDS_ZH if zh else ENDS_EN))
    text = "".join(parts)
    if seed % 5 == 0:
        text = "\n  " + text
    if seed % 7 == 0:
        text = text.rstrip()
    return text


def check_invariants(text, encode, max_tokens, pauses=Pauses()):
    segs = split_text(text, encode, max_tokens, pauses)
    assert "".join(s.text for s in segs) == text
    for s in segs:
        assert isinstance(s, Segment) and s.text.strip(), "a whitespace-only segment"
        assert s.tokens == list(encode(s.text.strip())) and 0 < len(s.tokens) <= max_tokens
        assert s.cut in CUTS + ("end",) and s.pause_ms == pauses.of(s.cut)
    assert segs[-1].cut == "end" and segs[-1].pause_ms == 0
    assert all(s.cut != "end" for s in segs[:-1])
    # a paragraph break always cuts
    for s in segs[:-1]:
        if "\n" in s.text.lstrip():
            assert s.text.rstrip(" \t\r\n") != s.text and "\n" not in s.text.strip() and s.cut == "paragraph"
    assert segs == split_text(text, encode, max_tokens, pauses)  # deterministic
    if len(encode(text.strip())) <= max_tokens and "\n" not in text.strip():
        assert len(segs) == 1
    return segs


@pytest.mark.parametrize("seed", range(60))
def test_invariants_with_the_tokenizer(tok, seed):
    text = generated(seed)
    for max_tokens in (8, 24, 64):
        check_invariants(text, tok.encode, max_tokens)


@pytest.mark.parametrize("seed", range(30))
def test_invariants_one_token_per_character(seed):
    text = generated(100 + seed)
    for max_tokens in (5, 17, 64, 10 ** 6):
        check_invariants(text, chars, max_tokens)


def texts(segs):
    return [(s.text, s.cut, s.pause_ms) for s in segs]


TABLE = [
    # within budget, no paragraph break: one segment
    ("Hello world. How are you?", 64, [("Hello world. How are you?", "end", 0)]),
    # sentences pack greedily while they fit
    ("One two. Three four. Five six. Seven.", 20,
     [("One two. Three four. ", "sentence", 300), ("Five six. Seven.", "end", 0)]),
    # a paragraph break always cuts, whatever fits
    ("Hi.\n\nBye.", 64, [("Hi.\n\n", "paragraph", 600), ("Bye.", "end", 0)]),
    # '.' inside a number or before a letter is no sentence end; closing quotes stay with the sentence
    ("Pi is 3.14 exactly. \"Really?\" he asked.", 21,
     [("Pi is 3.14 exactly. ", "sentence", 300), ("\"Really?\" he asked.", "end", 0)]),
    # a sentence over budget is cut at a clause, then at a space
    ("alpha beta, gamma delta epsilon zeta", 12,
     [("alpha beta, ", "clause", 150), ("gamma delta ", "whitespace", 60), ("epsilon zeta", "end", 0)]),
    # nothing to cut at: the longest prefix that fits
    ("abcdefghij", 4, [("abcd", "forced", 0), ("efgh", "forced", 0), ("ij", "end", 0)]),
    # Chinese: full-width terminators, no spaces
    ("今天天气很好。我们去公园吧！好的。", 8,
     [("今天天气很好。", "sentence", 300), ("我们去公园吧！", "sentence", 300), ("好的。", "end", 0)]),
    ("今天天气很好。我们去公园吧！好的。", 11,
     [("今天天气很好。", "sentence", 300), ("我们去公园吧！好的。", "end", 0)]),
    ("我们去公园散步，然后回家吃饭。", 9, [("我们去公园散步，", "clause", 150), ("然后回家吃饭。", "end", 0)]),
    ("他说：“明天见。”然后走了。", 9, [("他说：“明天见。”", "sentence", 300), ("然后走了。", "end", 0)]),
    # mixed
    ("RWKV 很快。It is fast!\n下一段……", 12,
     [("RWKV 很快。", "sentence", 300), ("It is fast!\n", "paragraph", 600), ("下一段……", "end", 0)]),
    # whitespace-only pieces join their neighbour; the larger pause stays
    ("\n\nHello.\n \n", 64, [("\n\nHello.\n \n", "end", 0)]),
    ("A b.   \n\n  C d.", 64, [("A b.   \n\n  ", "paragraph", 600), ("C d.", "end", 0)]),
]


@pytest.mark.parametrize("text,max_tokens,want", TABLE)
def test_examples(text, max_tokens, want):
    assert texts(check_invariants(text, chars, max_tokens)) == want


def test_pauses_are_parameters():
    p = Pauses(paragraph=1000, sentence=10, clause=5, whitespace=1, forced=2)
    segs = split_text("Aa bb, cc dd. Ee.\nFfffffffff", chars, 6, p)
    assert texts(segs) == [("Aa bb, ", "clause", 5), ("cc dd. ", "sentence", 10), ("Ee.\n", "paragraph", 1000),
                           ("Ffffff", "forced", 2), ("ffff", "end", 0)]


def test_empty_and_bad_arguments(tok):
    assert split_text("", tok.encode) == [] and split_text(" \n\t ", tok.encode) == []
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError):
            split_text("x", tok.encode, bad)
    with pytest.raises(ValueError):
        split_text("今天", lambda t: list(t.encode("utf-8")), 2)  # a single character needs 3 tokens
    with pytest.raises(Exception):
        split_text("\U0001F600", tok.encode)  # untokenisable text raises what encode raises
