"""Caption tokenizer: the reference numericalizes captions with nltk.tokenize.word_tokenize on the
lower-cased text (dataset.py:45-51, vocabulary.py:42-46). nltk (and its punkt model) is absent
here, so `word_tokenize` uses nltk when importable and otherwise this restatement of nltk's
Treebank word tokenizer rules (starting quotes, punctuation, brackets, double dashes, ending
quotes and clitics, the contraction splits), applied to the whole caption as one sentence.
Parity with nltk is unpinned (no nltk outputs are available); on plain COCO captions (words,
commas, a final period) the rules reduce to whitespace splitting with punctuation split off.
"""
import re
import unicodedata

_STARTING_QUOTES = [(re.compile(r'^\"'), r'``'), (re.compile(r'(``)'), r' \1 '),
                    (re.compile(r"([ \(\[{<])(\"|\'{2})"), r'\1 `` ')]
_PUNCTUATION = [
    (re.compile(r'([^\.])(\.)([\]\)}>"\']*)\s*$'), r'\1 \2 \3 '),
    (re.compile(r'([:,])([^\d])'), r' \1 \2'),
    (re.compile(r'([:,])$'), r' \1 '),
    (re.compile(r'\.\.\.'), r' ... '),
    (re.compile(r'[;@#$%&]'), r' \g<0> '),
    (re.compile(r'[?!]'), r' \g<0> '),
    (re.compile(r"([^'])' "), r"\1 ' "),
]
_PARENS = (re.compile(r'[\]\[\(\)\{\}\<\>]'), r' \g<0> ')
_DOUBLE_DASHES = (re.compile(r'--'), r' -- ')
_ENDING_QUOTES = [(re.compile(r'"'), " '' "), (re.compile(r"(\S)(\'\')"), r'\1 \2 '),
                  (re.compile(r"([^' ])('[sS]|'[mM]|'[dD]|') "), r'\1 \2 '),
                  (re.compile(r"([^' ])('ll|'LL|'re|'RE|'ve|'VE|n't|N'T) "), r'\1 \2 ')]
_CONTRACTIONS = [re.compile(p, re.I) for p in (
    r'\b(can)(not)\b', r"\b(d)('ye)\b", r'\b(gim)(me)\b', r'\b(gon)(na)\b', r'\b(got)(ta)\b',
    r'\b(lem)(me)\b', r"\b(more)('n)\b", r'\b(wan)(na)(?=\s)', r"('t)(is)\b", r"('t)(was)\b")]


def _treebank(text):
    for rx, sub in _STARTING_QUOTES:
        text = rx.sub(sub, text)
    for rx, sub in _PUNCTUATION:
        text = rx.sub(sub, text)
    text = _PARENS[0].sub(_PARENS[1], text)
    text = _DOUBLE_DASHES[0].sub(_DOUBLE_DASHES[1], text)
    text = ' ' + text + ' '
    for rx, sub in _ENDING_QUOTES:
        text = rx.sub(sub, text)
    for rx in _CONTRACTIONS:
        text = rx.sub(r' \1 \2 ', text)
    return text.split()


def word_tokenize(text):
    try:
        import nltk
        return nltk.tokenize.word_tokenize(text)
    except (ImportError, LookupError):  # no nltk, or no punkt model
        return _treebank(text)


# ======================================================================================
# BERT's uncased WordPiece tokenizer (what the reference's BertTokenizer.from_pretrained(
# 'bert-base-uncased').tokenize does to a caption, models/attention.py:172), dependency-free:
# basic tokenizer (whitespace split, lower-casing, accent stripping, punctuation split; no CJK
# spacing) then greedy longest-match WordPiece.
# ======================================================================================
NEVER_SPLIT = ("[UNK]", "[SEP]", "[PAD]", "[CLS]", "[MASK]")
MAX_CHARS_PER_WORD = 100


def _is_whitespace(ch):
    return ch in " \t\n\r" or unicodedata.category(ch) == "Zs"


def _is_control(ch):
    return ch not in "\t\n\r" and unicodedata.category(ch).startswith("C")


def _is_punctuation(ch):
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True  # all non-alphanumeric ASCII, as BERT treats it ('<', '>', '$', '^', '`' included)
    return unicodedata.category(ch).startswith("P")


def load_wordpiece_vocab(path):
    """vocab.txt (one piece per line, the line number is its id) -> {piece: id}."""
    vocab = {}
    with open(path, encoding="utf-8") as f:
        for i, line in enumerate(f):
            vocab[line.rstrip("\n")] = i
    return vocab


class WordPieceTokenizer:
    """``tokenize(text)`` -> pieces, ``convert_tokens_to_ids(pieces)`` -> ids, for an uncased BERT vocabulary
    (``vocab``: a vocab.txt path or a {piece: id} dict)."""

    def __init__(self, vocab, unk_token="[UNK]", never_split=NEVER_SPLIT):
        self.vocab = load_wordpiece_vocab(vocab) if isinstance(vocab, (str, bytes)) or hasattr(vocab, "__fspath__") \
            else dict(vocab)
        self.unk_token = unk_token
        self.never_split = set(never_split)
        if unk_token not in self.vocab:
            raise ValueError(f"WordPiece vocabulary has no {unk_token}")

    def basic_tokenize(self, text):
        text = "".join(" " if _is_whitespace(c) else c for c in text
                       if not (ord(c) == 0 or ord(c) == 0xFFFD or _is_control(c)))
        out = []
        for tok in text.split():
            if tok in self.never_split:
                out.append(tok)
                continue
            tok = "".join(c for c in unicodedata.normalize("NFD", tok.lower()) if unicodedata.category(c) != "Mn")
            word = ""
            for c in tok:  # every punctuation character is a token of its own
                if _is_punctuation(c):
                    if word:
                        out.append(word)
                    out.append(c)
                    word = ""
                else:
                    word += c
            if word:
                out.append(word)
        return out

    def wordpiece(self, word):
        if len(word) > MAX_CHARS_PER_WORD:
            return [self.unk_token]
        pieces, start = [], 0
        while start < len(word):
            end = len(word)
            while end > start:
                sub = ("##" if start > 0 else "") + word[start:end]
                if sub in self.vocab:
                    break
                end -= 1
            if end == start:
                return [self.unk_token]
            pieces.append(sub)
            start = end
        return pieces

    def tokenize(self, text):
        out = []
        for tok in self.basic_tokenize(text):
            out.extend([tok] if tok in self.never_split else self.wordpiece(tok))
        return out

    def convert_tokens_to_ids(self, pieces):
        return [self.vocab[p] for p in pieces]

    def encode_word(self, word):
        return self.convert_tokens_to_ids(self.tokenize(word))


def word_pieces(vocabulary, tokenizer):
    """The piece ids of every caption-vocabulary word, as a CSR pair (offsets int64 [V + 1], ids int32): word
    index i owns ids[offsets[i]:offsets[i+1]]. BERT tokenizes whitespace-separated words independently, so the
    pieces of ' '.join(words) are the concatenation of the words' pieces; '<pad>', '<start>', '<end>' and
    '<unk>' are ordinary text ('<', 'pad', '>'), as in the reference (models/attention.py:169-172)."""
    import numpy as np
    V = len(vocabulary)
    offsets = np.zeros(V + 1, dtype=np.int64)
    ids = []
    for i in range(V):
        ids.extend(tokenizer.encode_word(vocabulary.i2w[i]))
        offsets[i + 1] = len(ids)
    return offsets, np.asarray(ids, dtype=np.int32)
