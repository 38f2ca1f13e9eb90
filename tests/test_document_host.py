"""datasets/document.py on the CPU: the number table of expand_numbers and the rules of split_document."""
import random

import pytest

from tacotron2_amd.datasets.document import ABBREVIATIONS, Piece, expand_numbers, split_document
from tacotron2_amd.datasets.text import TextEncoder

NUMBERS = [("0", "zero"), ("7", "seven"), ("13", "thirteen"), ("20", "twenty"), ("21", "twenty one"), ("100", "one hundred"),
           ("101", "one hundred one"), ("1,000", "one thousand"), ("1,234", "one thousand two hundred thirty four"),
           ("1000000", "one million"), ("999999999999999", "nine hundred ninety nine trillion nine hundred ninety nine billion nine hundred "
                                                           "ninety nine million nine hundred ninety nine thousand nine hundred ninety nine"),
           ("1234567890123456", "one two three four five six seven eight nine zero one two three four five six"),
           ("3.14", "three point one four"), ("0.5", "zero point five"), ("1st", "first"), ("2nd", "second"), ("3rd", "third"),
           ("11th", "eleventh"), ("22nd", "twenty second"), ("103rd", "one hundred third"), ("40th", "fortieth"), ("100th", "one hundredth"),
           ("-5", "minus five"), ("50%", "fifty percent"), ("-2.5%", "minus two point five percent"), ("1,000,000", "one million"),
           ("B52", "B52"), ("5kg", "5kg"), ("1.2.3", "1.2.3"), ("12:30", "12:30"), ("1th", "1th"), ("1,23", "1,23"), ("x2", "x2")]


@pytest.mark.parametrize("text,want", NUMBERS, ids=[n[0] for n in NUMBERS])
def test_the_number_table(text, want):
    assert expand_numbers(text) == want
    assert expand_numbers(f"In {text}, then.") == f"In {want}, then."


def test_numbers_in_a_sentence():
    assert expand_numbers("In 1984, 3 men") == "In one thousand nine hundred eighty four, three men"       # (years are not built)
    assert expand_numbers("Pages 3-5 cost 7.") == "Pages three-five cost seven."
    assert expand_numbers("It fell to (-5) or -5.") == "It fell to (minus five) or minus five."
    assert expand_numbers("no digits here") == "no digits here"
    enc = TextEncoder()
    assert enc.clean("In 1984, 3 men") == "in ,  men^" and enc.clean(expand_numbers("3 men")) == "three men^"


def _texts(pieces):
    return [p.text for p in pieces]


def test_sentence_ends():
    assert len(ABBREVIATIONS) == 18 and "dr" in ABBREVIATIONS and "mrs" in ABBREVIATIONS
    p = split_document("Dr. Smith met Mrs. Jones. They talked.")
    assert p == [Piece("Dr. Smith met Mrs. Jones.", 0, "sentence"), Piece("They talked.", 0, "end")]
    assert _texts(split_document("DR. Smith and st. Louis. Yes.")) == ["DR. Smith and st. Louis.", "Yes."]
    assert _texts(split_document("J. R. R. Tolkien wrote it. So.")) == ["J. R. R. Tolkien wrote it.", "So."]
    assert _texts(split_document("Pi is 3.14 exactly. And 2. 5 is next.")) == ["Pi is 3.14 exactly.", "And 2.", "5 is next."]
    assert _texts(split_document("What?! No... Yes!")) == ["What?!", "No...", "Yes!"]
    assert _texts(split_document('He said "go." She said (no!) Then left.')) == ['He said "go."', "She said (no!)", "Then left."]
    assert _texts(split_document("a.b is one. No stop at the end")) == ["a.b is one.", "No stop at the end"]
    assert _texts(split_document("Dr. Smith.", abbreviations=())) == ["Dr.", "Smith."]
    assert split_document("") == [] and split_document(" \n\n \n") == []


def test_paragraphs():
    p = split_document("One. Two.\n\nThree.\n \n\n  Four\nfive.\r\n\r\nSix.")
    assert p == [Piece("One.", 0, "sentence"), Piece("Two.", 0, "paragraph"), Piece("Three.", 1, "paragraph"),
                 Piece("Four five.", 2, "paragraph"), Piece("Six.", 3, "end")]


def test_the_cap():
    s = "alpha beta; gamma delta, epsilon zeta eta theta."
    assert split_document(s, max_chars=100) == [Piece(s, 0, "end")]
    assert split_document(s, max_chars=30) == [Piece("alpha beta; gamma delta,", 0, "clause"), Piece("epsilon zeta eta theta.", 0, "end")]
    assert _texts(split_document(s, max_chars=20)) == ["alpha beta;", "gamma delta,", "epsilon zeta eta", "theta."]       # ';', ',', a space
    assert _texts(split_document(s, max_chars=11)) == ["alpha beta;", "gamma", "delta,", "epsilon", "zeta eta", "theta."]
    assert _texts(split_document("a,b c,d e", max_chars=5)) == ["a,b", "c,d e"]             # a ',' without a space behind it is no cut
    with pytest.raises(ValueError, match="'" + "x" * 40 + "'"):
        split_document("short " + "x" * 60 + " words", max_chars=50)
    with pytest.raises(ValueError, match="max_chars"):
        split_document("a", max_chars=0)


def test_the_cap_counts_cleaned_characters():
    s = "12345 67890 abc 12345 def."                        # cleaned: "  abc  def." - 11 characters
    assert len(TextEncoder(end_token=None).clean(s)) == 11
    assert split_document(s, max_chars=11) == [Piece(s, 0, "end")]
    assert _texts(split_document(s, max_chars=10)) == ["12345 67890 abc 12345", "def."]
    clean = TextEncoder("abc ", end_token="^").clean        # another alphabet: the caller's encoder decides
    assert _texts(split_document("abc xyz xyz abc abc", max_chars=9, clean=lambda t: clean(t)[:-1])) == ["abc xyz xyz abc", "abc"]


def test_dropped_pieces_pass_their_break_upward():
    p = split_document("First one. ***\n\nNext. Then.\n\n— — —\n\nLast, here.\n\n***")
    assert p == [Piece("First one.", 0, "paragraph"), Piece("Next.", 1, "sentence"), Piece("Then.", 1, "paragraph"),
                 Piece("Last, here.", 3, "end")]
    assert split_document("*** 123") == []
    assert split_document("***\n\nOnly.") == [Piece("Only.", 1, "end")]
    p = split_document("alpha beta, *** gamma.", max_chars=12)
    assert p == [Piece("alpha beta,", 0, "clause"), Piece("*** gamma.", 0, "end")]
    assert split_document("One. *** Two.") == [Piece("One.", 0, "sentence"), Piece("*** Two.", 0, "end")]
    assert split_document("One. ***! Two.") == [Piece("One.", 0, "sentence"), Piece("***!", 0, "sentence"), Piece("Two.", 0, "end")]


WORDS = ["a", "I", "Dr.", "Mr.", "J.", "3.14", "1,234", "***", "the", "quick", "brown;", "fox,", "jumps:", "over", "lazy", "dog.", "dog!",
         'dog."', "why?!", "antidisestablishmentarianism", "(so)", "\n\n", "\n \n", "  ", "\t", "—", "naïve", "1984,"]


@pytest.mark.parametrize("seed", range(8))
def test_rejoining_the_pieces_gives_the_text_back(seed):
    rng = random.Random(seed)
    text = "".join(rng.choice(WORDS) + rng.choice([" ", " ", "  ", "\n"]) for _ in range(300))
    clean = TextEncoder(end_token=None).clean
    for cap in (28, 60, 190):
        pieces = split_document(text, max_chars=cap)
        assert pieces[-1].break_after == "end" and all(p.break_after != "end" for p in pieces[:-1])
        assert all(len(clean(p.text)) <= cap and clean(p.text).strip() for p in pieces)
        assert [p.paragraph_index for p in pieces] == sorted(p.paragraph_index for p in pieces)
        # with a cleaner that deletes nothing, nothing is dropped: the pieces ARE the text
        whole = split_document(text, max_chars=cap, clean=lambda t: "".join(" " if c.isspace() else "x" for c in t))
        assert " ".join(_texts(whole)) == " ".join(text.split())
        # with the encoder's: the pieces' words are the text's words in order, and every word left out cleans to nothing
        got, i = " ".join(_texts(pieces)).split(" "), 0
        for t in " ".join(text.split()).split(" "):
            if i < len(got) and got[i] == t:
                i += 1
            else:
                assert not clean(t).strip(), t
        assert i == len(got)
