"""Deterministic text segmentation for long-form synthesis (no reference counterpart: the reference
hands a whole text to one request, which stops at 2048 semantic tokens). Host only.

split_text(text, encode, max_tokens=64, pauses=Pauses()) cuts a text into segments whose encodings
fit max_tokens text tokens each, at the best boundary available, and gives each the pause that
follows it. Cut classes, by preference:

    paragraph   a run of newlines (with the blanks around it)
    sentence    after one of 。！？!?… , or after '.' followed by whitespace or the end; closing quotes
                and brackets that follow stay with the sentence
    clause      after one of ，,；;：:、 (an ASCII ',' or ':' between two digits is no boundary)
    whitespace  at a space
    forced      the longest character prefix whose encoding fits

Packing is greedy: consecutive sentences merge while their encoding stays within max_tokens; a
paragraph break always cuts; a sentence over budget is cut by the next class down, again greedily.
What holds for every result (tests/test_segment.py):

    "".join(s.text for s in segments) == text          (for a text that is not whitespace only)
    len(encode(s.text.strip())) <= max_tokens, and s.tokens is that encoding
    no segment is whitespace only (its pause merges into the previous segment's as the maximum)
    a text within budget and without a paragraph break is exactly one segment
    the result depends on (text, encode, max_tokens, pauses) alone

max_tokens = 64 and the pauses are defaults nobody has measured on a real checkpoint (DESIGN.md
§23): the zero-shot heuristic assumes >= 1.8 semantic tokens per text token, speech at 50 semantic
tokens per second suggests roughly 10-12, so 64 text tokens leave about 3x headroom under 2048.
"""
import dataclasses
from typing import Callable, List, Sequence

SENTENCE_END = "。！？!?…"
CLOSERS = "\"'”’」』）)]】》〉»"
CLAUSE_END = "，,；;：:、"
CUTS = ("paragraph", "sentence", "clause", "whitespace", "forced")
_FORCED_LOOKAHEAD = 32  # characters past the monotone answer that the forced cut still tries


@dataclasses.dataclass(frozen=True)
class Pauses:
    """Milliseconds of silence after a segment, by the class of the cut that ends it."""
    paragraph: int = 600
    sentence: int = 300
    clause: int = 150
    whitespace: int = 60
    forced: int = 0

    def of(self, cut: str) -> int:
        return 0 if cut == "end" else int(getattr(self, cut))


@dataclasses.dataclass
class Segment:
    text: str          # the segment with its surrounding whitespace: the texts concatenate to the input
    tokens: List[int]  # encode(text.strip())
    pause_ms: int      # from the cut after the segment; 0 for the last one
    cut: str           # the class of that cut: one of CUTS, or "end"


def _is_space(c: str) -> bool:
    return c.isspace()


def _paragraphs(text: str) -> List[str]:
    """Pieces ending with a maximal run of whitespace that holds a newline."""
    out, i, start, n = [], 0, 0, len(text)
    while i < n:
        if text[i] == "\n":
            j = i
            while j < n and _is_space(text[j]):
                j += 1
            out.append(text[start:j])
            start = i = j
        else:
            i += 1
    if start < n:
        out.append(text[start:])
    return out


def _sentences(text: str) -> List[str]:
    out, i, start, n = [], 0, 0, len(text)
    while i < n:
        c = text[i]
        if c in SENTENCE_END or c == ".":
            j, hard = i, False
            while j < n and (text[j] in SENTENCE_END or text[j] == "."):
                hard |= text[j] in SENTENCE_END
                j += 1
            k = j
            while k < n and text[k] in CLOSERS:
                k += 1
            if hard or k == n or _is_space(text[k]):
                while k < n and _is_space(text[k]):
                    k += 1
                out.append(text[start:k])
                start = i = k
                continue
            i = j
        else:
            i += 1
    if start < n:
        out.append(text[start:])
    return out


def _clauses(text: str) -> List[str]:
    out, i, start, n = [], 0, 0, len(text)
    while i < n:
        c = text[i]
        between_digits = c in ",:" and 0 < i < n - 1 and text[i - 1].isdigit() and text[i + 1].isdigit()
        if c in CLAUSE_END and not between_digits:
            k = i + 1
            while k < n and (text[k] in CLAUSE_END or _is_space(text[k])):
                k += 1
            out.append(text[start:k])
            start = i = k
        else:
            i += 1
    if start < n:
        out.append(text[start:])
    return out


def _words(text: str) -> List[str]:
    out, i, start, n = [], 0, 0, len(text)
    while i < n:
        if _is_space(text[i]):
            k = i
            while k < n and _is_space(text[k]):
                k += 1
            out.append(text[start:k])
            start = i = k
        else:
            i += 1
    if start < n:
        out.append(text[start:])
    return out


_SPLITTERS = {"sentence": _sentences, "clause": _clauses, "whitespace": _words}
_NEXT = {"sentence": "clause", "clause": "whitespace", "whitespace": "forced"}


def _forced(text: str, fits) -> List[str]:
    """Greedy prefixes: the longest that fits by bisection (a prefix's token count grows with it, up
    to merges at its end), then up to _FORCED_LOOKAHEAD characters further for a longer one that a
    merge lets fit."""
    out = []
    while text:
        if fits(text):
            out.append(text)
            break
        if not fits(text[:1]):
            raise ValueError("split_text: max_tokens is too small for a single character")
        lo, hi = 1, len(text)  # lo fits, hi does not
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if fits(text[:mid]):
                lo = mid
            else:
                hi = mid
        for k in range(min(len(text) - 1, lo + _FORCED_LOOKAHEAD), lo, -1):
            if fits(text[:k]):
                lo = k
                break
        out.append(text[:lo])
        text = text[lo:]
    return out


def _pack(text: str, final_cut: str, level: str, fits) -> list:
    """-> [(piece, cut class after it)], the pieces concatenating to text, the last cut final_cut."""
    if fits(text):
        return [(text, final_cut)]
    if level == "forced":
        pieces = _forced(text, fits)
        return [(p, "forced") for p in pieces[:-1]] + [(pieces[-1], final_cut)]
    out, cur = [], ""
    for atom in _SPLITTERS[level](text):
        if fits(cur + atom):
            cur += atom
            continue
        if cur:
            out.append((cur, level))
            cur = ""
        if fits(atom):
            cur = atom
        else:  # the atom alone is over budget: the next class down; its last piece may still grow
            sub = _pack(atom, level, _NEXT[level], fits)
            out.extend(sub[:-1])
            cur = sub[-1][0]
    if cur:
        out.append((cur, final_cut))
    return out


def split_text(text: str, encode: Callable[[str], Sequence[int]], max_tokens: int = 64,
               pauses: Pauses = Pauses()) -> List[Segment]:
    """See the module docstring. encode: text -> token ids (Tokenizer.encode); a text it cannot
    encode raises what encode raises. A text that is empty or whitespace only gives no segment."""
    if isinstance(max_tokens, bool) or not isinstance(max_tokens, int) or max_tokens < 1:
        raise ValueError("split_text: max_tokens must be an integer >= 1")
    if not text.strip():
        return []
    cache = {}

    def count(t: str) -> int:
        t = t.strip()
        if t not in cache:
            cache[t] = len(encode(t)) if t else 0
        return cache[t]

    def fits(t: str) -> bool:
        return count(t) <= max_tokens

    pieces = []
    pars = _paragraphs(text)
    for i, par in enumerate(pars):
        pieces.extend(_pack(par, "paragraph" if i + 1 < len(pars) else "end", "sentence", fits))
    # no segment is whitespace only: it joins the segment before it (the first one: the one after it)
    merged, lead = [], ""
    for t, cut in pieces:
        if not t.strip():
            if merged:
                pt, pcut = merged[-1]
                merged[-1] = (pt + t, cut if pauses.of(cut) > pauses.of(pcut) or cut == "end" else pcut)
            else:
                lead += t
            continue
        merged.append((lead + t, cut))
        lead = ""
    if merged:
        merged[-1] = (merged[-1][0], "end")
    return [Segment(t, [int(x) for x in encode(t.strip())], pauses.of(cut), cut) for t, cut in merged]
