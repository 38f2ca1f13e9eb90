"""A document for `say --text-file`: numbers into words (opt-in) and the text into pieces the model was trained on - sentences of
at most max_chars characters -, each with the kind of break that follows it.  Host only, pure Python, English only."""
from __future__ import annotations

import re
from typing import Callable, List, NamedTuple, Optional, Sequence

from .text import _ABBREVIATIONS, ALLOWED_CHARS, TextEncoder

ABBREVIATIONS = tuple(rx.pattern[2:-2] for rx, _ in _ABBREVIATIONS)          # the 18 of datasets/text.py: "mrs", "mr", "dr", ...
BREAKS = ("clause", "sentence", "paragraph", "end")                           # in ascending strength

_ONES = ("zero one two three four five six seven eight nine ten eleven twelve thirteen fourteen fifteen sixteen seventeen eighteen "
         "nineteen").split()
_TENS = "zero ten twenty thirty forty fifty sixty seventy eighty ninety".split()
_SCALES = ("", "thousand", "million", "billion", "trillion")
_ORDINALS = dict(one="first", two="second", three="third", five="fifth", eight="eighth", nine="ninth", twelve="twelfth")
_NUMBER = re.compile(r"(?<![\w.,:/])(?P<minus>(?<![\w\-])-)?(?P<int>\d{1,3}(?:,\d{3})+|\d+)(?P<frac>\.\d+)?(?P<ord>st|nd|rd|th)?(?P<pct>%)?"
                     r"(?![\w])(?![.,:/]\d)")


def _below_1000(n: int) -> List[str]:
    out = [_ONES[n // 100], "hundred"] if n >= 100 else []
    n %= 100
    if n >= 20:
        out += [_TENS[n // 10]] + ([_ONES[n % 10]] if n % 10 else [])
    elif n:
        out.append(_ONES[n])
    return out


def _cardinal(n: int) -> List[str]:
    if n == 0:
        return ["zero"]
    groups, out = [], []
    while n:
        groups.append(n % 1000)
        n //= 1000
    for k in range(len(groups) - 1, -1, -1):
        if groups[k]:
            out += _below_1000(groups[k]) + ([_SCALES[k]] if k else [])
    return out


def _ordinal(n: int) -> List[str]:
    w = _cardinal(n)
    last = w[-1]
    w[-1] = _ORDINALS.get(last) or (last[:-1] + "ieth" if last.endswith("y") else last + "th")
    return w


def _suffix(n: int) -> str:
    return "th" if 10 <= n % 100 <= 20 else {1: "st", 2: "nd", 3: "rd"}.get(n % 10, "th")


def expand_numbers(text: str) -> str:
    """Numbers of an English text into words, before TextEncoder.clean deletes every digit.  Opt-in (`say --expand-numbers`).

        input                          output                                     rule
        0, 7, 13, 20, 21, 101          zero, seven, thirteen, twenty, twenty one, integers up to 10^15 - 1: groups of three with
                                       one hundred one                            thousand / million / billion / trillion; no "and",
        1,234  1000000                 one thousand two hundred thirty four,      no hyphens; thousands commas (groups of exactly
                                       one million                                three digits) are read through
        3.14   0.5                     three point one four, zero point five      decimals: the fraction digit by digit
        1st 2nd 3rd 11th 22nd 103rd    first second third eleventh twenty second  ordinals: an integer with ITS English suffix (a
                                       one hundred third                          wrong one, 1th, is left alone)
        -5                             minus five                                 a '-' in front of a number at a word start (start
                                                                                  of the text, or behind whitespace or a bracket)
        50%                            fifty percent                              a trailing '%'
        1234567890123456               one two three ... six                      a run of more than 15 digits: digit by digit
        B52  5kg  1.2.3  12:30         unchanged                                  a number glued to a letter, or inside a longer
                                                                                  run of digits and stops, is left as it is -
                                                                                  TextEncoder then drops its digits, as before

    NOT built: years (1984 is "one thousand nine hundred eighty four"), currency ($5 is "$five": the sign is deleted by the
    encoder), clock times, Roman numerals, fractions (1/2), ranges, and any language but English."""
    def words(m: "re.Match") -> str:
        digits = m.group("int").replace(",", "")
        if m.group("ord"):
            if m.group("frac") or len(digits) > 15 or m.group("ord") != _suffix(int(digits)):
                return m.group(0)
            w = _ordinal(int(digits))
        elif len(digits) > 15:
            w = [_ONES[int(d)] for d in digits]
        else:
            w = _cardinal(int(digits))
        if m.group("frac"):
            w += ["point"] + [_ONES[int(d)] for d in m.group("frac")[1:]]
        return ("minus " if m.group("minus") else "") + " ".join(w) + (" percent" if m.group("pct") else "")
    return _NUMBER.sub(words, text)


class Piece(NamedTuple):
    text: str
    paragraph_index: int
    break_after: str            # one of BREAKS


_CLOSERS = "\"')\\]”’»"
_SENTENCE_END = re.compile(rf"[.!?]+[{_CLOSERS}]*(?=\s|$)")
_INITIAL = re.compile(r"(?<![A-Za-z])[A-Z]$")


def _default_clean() -> Callable[[str], str]:
    return TextEncoder(ALLOWED_CHARS, end_token=None).clean


def _sentences(par: str, abbreviations: Sequence[str]) -> List[str]:
    """The sentences of one paragraph with its whitespace runs already collapsed."""
    abbr = re.compile(r"\b(?:%s)$" % "|".join(re.escape(a) for a in abbreviations), re.IGNORECASE) if abbreviations else None
    out, start = [], 0
    for m in _SENTENCE_END.finditer(par):
        stops = m.group(0).rstrip(_CLOSERS.replace("\\", ""))
        if stops == ".":
            before = par[start:m.start()]
            if (abbr is not None and abbr.search(before)) or _INITIAL.search(before):
                continue                                    # "Dr. Smith", "J. R. R. Tolkien"
            if before[-1:].isdigit() and par[m.end():m.end() + 1].isdigit():
                continue                                    # between two digits (3.14 has no whitespace behind the stop anyway)
        out.append(par[start:m.end()])
        start = m.end() + 1                                 # (one space, or the end)
    if start < len(par):
        out.append(par[start:])
    return out


def _cut(sentence: str, max_chars: int, clean: Callable[[str], str]) -> List[str]:
    """A sentence as pieces of at most max_chars CLEANED characters: cut behind the last ';', ':' or ',' that a space follows, else
    at the last space."""
    out = []
    while True:
        cum = [0]                                           # cum[k] = cleaned characters of sentence[:k]
        for ch in sentence:
            cum.append(cum[-1] + len(clean(ch)))
        if cum[-1] <= max_chars:
            return out + [sentence]
        fits = [k for k in range(1, len(sentence)) if sentence[k] == " " and cum[k] <= max_chars]
        if not fits:
            word = sentence.split(" ", 1)[0]
            raise ValueError(f"split_document: a word of more than max_chars = {max_chars} characters: {word[:40]!r}")
        marks = [k for k in fits if sentence[k - 1] in ";:,"]
        k = (marks or fits)[-1]
        out.append(sentence[:k])
        sentence = sentence[k + 1:]


def split_document(text: str, max_chars: int = 190, abbreviations: Sequence[str] = ABBREVIATIONS,
                   clean: Optional[Callable[[str], str]] = None) -> List[Piece]:
    """A text as the pieces `say --text-file` decodes side by side: Piece(text, paragraph_index, break_after), break_after one of
    "clause", "sentence", "paragraph", "end".

    - A blank line ends a paragraph.
    - A sentence ends at '.', '!' or '?' (a run of them: "?!", "..."), optionally followed by closing quotes or brackets, followed
      by whitespace or the end of the text.  A single '.' does not end one directly behind one of `abbreviations` (the 18 of
      datasets/text.py, any case: "Dr. Smith"), behind a single capital letter ("J. R. R. Tolkien" - and so, wrongly, not behind
      "So did I."), or between two digits.
    - max_chars counts the characters of the CLEANED text (`clean`: TextEncoder.clean without the end token; default: the default
      alphabet), which is what the model sees.  A longer sentence is cut behind the last ';', ':' or ',' at or before the cap that a
      space follows (break "clause"), else at the last space (also "clause"); a single word above the cap is a ValueError that
      quotes its first 40 characters.
    - A piece that cleans to nothing ("***", a row of dashes) is dropped; the stronger of its break and its predecessor's stays
      with the predecessor.  The last surviving piece has the break "end".
    - " ".join of the pieces' texts is the input with its whitespace runs collapsed, minus the dropped pieces."""
    if isinstance(max_chars, bool) or not isinstance(max_chars, int) or max_chars < 1:
        raise ValueError(f"split_document: max_chars must be an integer >= 1, got {max_chars!r}")
    clean = clean or _default_clean()
    pieces: List[Piece] = []
    pars = [" ".join(p.split()) for p in re.split(r"\n[^\S\n]*\n\s*", text.replace("\r\n", "\n").replace("\r", "\n"))]
    for pi, par in enumerate(p for p in pars if p):
        found = []
        for s in _sentences(par, abbreviations):
            cut = _cut(s, max_chars, clean)
            found += [(c, "clause") for c in cut[:-1]] + [(cut[-1], "sentence")]
        found[-1] = (found[-1][0], "paragraph")
        for t, brk in found:
            if clean(t).strip():
                pieces.append(Piece(t, pi, brk))
            elif pieces and BREAKS.index(brk) > BREAKS.index(pieces[-1].break_after):
                pieces[-1] = pieces[-1]._replace(break_after=brk)
    if pieces:
        pieces[-1] = pieces[-1]._replace(break_after="end")
    return pieces
