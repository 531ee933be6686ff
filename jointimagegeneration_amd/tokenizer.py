"""BERT's WordPiece tokenizer on the host, in plain Python: what `AutoTokenizer.from_pretrained(dir)(texts, truncation=True,
max_length=L, padding="max_length")` gives for a BERT directory (vocab.txt + tokenizer_config.json), without transformers or tokenizers.

  basic tokenisation   special tokens ([UNK] [CLS] [SEP] [PAD] [MASK]) are cut out of the raw text first and never split or normalised;
                       the rest: control characters dropped, every whitespace character a space, CJK ideographs isolated, then -- with
                       do_lower_case -- lower-cased and stripped of accents (NFD, category Mn dropped), split on whitespace and around
                       every punctuation character
  WordPiece            greedy longest match from the left, continuation pieces carry the ## prefix; a word of more than 100 characters,
                       or one with a stretch no piece covers, is [UNK]
  encode               [CLS] pieces [SEP], cut to max_length keeping both ends, padded with [PAD]; the mask is 1 on real tokens
"""
from __future__ import annotations

import unicodedata
from typing import Dict, List, Sequence, Tuple

SPECIALS = ("[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]")
MAX_INPUT_CHARS_PER_WORD = 100


def _is_whitespace(ch: str) -> bool:
    return ch in " \t\n\r" or unicodedata.category(ch) == "Zs"


def _is_control(ch: str) -> bool:
    return ch not in "\t\n\r" and unicodedata.category(ch).startswith("C")


def _is_punctuation(ch: str) -> bool:
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:       # every non-alphanumeric ASCII character, $ and ^ too
        return True
    return unicodedata.category(ch).startswith("P")


def _is_cjk(cp: int) -> bool:
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


class BertWordPieceTokenizer:
    def __init__(self, vocab: Sequence[str], do_lower_case: bool = True):
        self.vocab: Dict[str, int] = {}
        for i, tok in enumerate(vocab):
            self.vocab.setdefault(tok, i)
        missing = [t for t in ("[UNK]", "[CLS]", "[SEP]", "[PAD]") if t not in self.vocab]
        if missing:
            raise ValueError(f"BertWordPieceTokenizer: the vocabulary lacks {missing}")
        self.do_lower_case = bool(do_lower_case)
        self.specials = tuple(t for t in SPECIALS if t in self.vocab)
        self.unk, self.cls, self.sep, self.pad = (self.vocab[t] for t in ("[UNK]", "[CLS]", "[SEP]", "[PAD]"))

    # ---- basic tokenisation
    def _split_specials(self, text: str) -> List[Tuple[str, bool]]:
        """[(piece, is_special)]: at each position the first special token that starts there is cut out."""
        out, start, i = [], 0, 0
        while i < len(text):
            hit = next((s for s in self.specials if text.startswith(s, i)), None) if text[i] == "[" else None
            if hit is None:
                i += 1
                continue
            if i > start:
                out.append((text[start:i], False))
            out.append((hit, True))
            i += len(hit)
            start = i
        if start < len(text):
            out.append((text[start:], False))
        return out

    def _words(self, text: str) -> List[str]:
        chars = []
        for ch in text:
            cp = ord(ch)
            if cp == 0 or cp == 0xFFFD or _is_control(ch):
                continue
            if _is_whitespace(ch):
                chars.append(" ")
            elif _is_cjk(cp):
                chars += [" ", ch, " "]
            else:
                chars.append(ch)
        text = "".join(chars)
        if self.do_lower_case:
            text = "".join(c for c in unicodedata.normalize("NFD", text) if unicodedata.category(c) != "Mn").lower()
        words: List[str] = []
        for tok in text.split():
            cur = ""
            for ch in tok:
                if _is_punctuation(ch):
                    if cur:
                        words.append(cur)
                    words.append(ch)
                    cur = ""
                else:
                    cur += ch
            if cur:
                words.append(cur)
        return words

    # ---- WordPiece
    def _wordpiece(self, word: str) -> List[int]:
        if len(word) > MAX_INPUT_CHARS_PER_WORD:
            return [self.unk]
        ids, start = [], 0
        while start < len(word):
            end, cur = len(word), None
            while start < end:
                piece = ("##" if start else "") + word[start:end]
                if piece in self.vocab:
                    cur = self.vocab[piece]
                    break
                end -= 1
            if cur is None:
                return [self.unk]
            ids.append(cur)
            start = end
        return ids

    def tokenize_ids(self, text: str) -> List[int]:
        """token ids of `text` without [CLS] / [SEP]"""
        ids: List[int] = []
        for piece, special in self._split_specials(text):
            if special:
                ids.append(self.vocab[piece])
            else:
                for w in self._words(piece):
                    ids += self._wordpiece(w)
        return ids

    def encode(self, texts: Sequence[str], max_length: int) -> Tuple[List[List[int]], List[List[int]]]:
        """(ids, mask), each [len(texts)][max_length]: [CLS] ... [SEP] truncated to max_length, [PAD]-padded; mask 1 on real tokens."""
        if max_length < 2:
            raise ValueError(f"BertWordPieceTokenizer: max_length = {max_length} leaves no room for [CLS] and [SEP]")
        all_ids, all_mask = [], []
        for t in texts:
            if not isinstance(t, str):
                raise TypeError(f"BertWordPieceTokenizer: texts must be str, got {type(t).__name__}")
            ids = [self.cls] + self.tokenize_ids(t)[:max_length - 2] + [self.sep]
            n = len(ids)
            all_ids.append(ids + [self.pad] * (max_length - n))
            all_mask.append([1] * n + [0] * (max_length - n))
        return all_ids, all_mask
