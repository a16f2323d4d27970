"""core/bloombits over batches, on the GPU: the section generator and what a Matcher session computes.

    Generator.AddBloom / Bitset     core/bloombits/generator.go:52-87
    NewMatcher                      core/bloombits/matcher.go:92-131
    a session's matches             core/bloombits/matcher.go:182-211, :337-366

The table of a run of sections is a (n_sections, 2048, section_size // 8) uint8 array: row `bit` of a section is
Generator.Bitset(bit).  The matcher's scheduler, distributor and retrieval sessions (database plumbing) have no
counterpart: a Matcher is run over a table the caller holds, and blocks outside the table are not reported.
"""
from __future__ import annotations

import numpy as np

from . import _lib, default_context


class ErrSectionOutOfBounds(ValueError):
    def __init__(self):
        super().__init__("section out of bounds")  # generator.go:27


class ErrSectionCount(ValueError):
    def __init__(self):
        super().__init__("section count not multiple of 8")  # generator.go:41


class ErrUnexpectedIndex(ValueError):
    def __init__(self):
        super().__init__("bloom filter with unexpected index")  # generator.go:58


class ErrNotGenerated(ValueError):
    def __init__(self):
        super().__init__("bloom not fully generated yet")  # generator.go:81


def _check_section(sections: int):
    if sections % 8:
        raise ErrSectionCount()
    if not 8 <= sections <= _lib.BLOOMBITS_MAX_SECTION:
        raise ValueError(f"bloombits: a section of {sections} blooms is outside 8 .. {_lib.BLOOMBITS_MAX_SECTION}")


class Generator:
    """bloombits.Generator: collects the section's blooms on the host and rotates them in one device call at the
    first Bitset."""

    def __init__(self, sections: int, ctx=None):
        self.sections = int(sections)
        self.nextBit = 0
        self._ctx = ctx
        self._blooms = np.zeros((self.sections, 256), np.uint8)
        self._bits = None

    def AddBloom(self, index: int, bloom):
        if self.nextBit >= self.sections:
            raise ErrSectionOutOfBounds()
        if self.nextBit != index:
            raise ErrUnexpectedIndex()
        row = np.frombuffer(bytes(bloom), np.uint8)
        if row.size != 256:
            raise ValueError("a Bloom is 256 bytes")
        self._blooms[self.nextBit] = row
        self.nextBit += 1

    def Bitset(self, idx: int) -> bytes:
        if self.nextBit != self.sections:
            raise ErrNotGenerated()
        if idx >= self.sections:  # generator.go:83-85 compares with the section size
            raise ErrSectionOutOfBounds()
        if self._bits is None:
            self._bits = (self._ctx or default_context()).bloombits_generate_batch(self._blooms, self.sections)[0]
        return self._bits[idx].tobytes()


def NewGenerator(sections: int, ctx=None) -> Generator:
    _check_section(int(sections))
    return Generator(sections, ctx)


def GenerateSections(blooms, section_size: int, ctx=None) -> np.ndarray:
    """the table of len(blooms) / section_size whole sections: (n_sections, 2048, section_size // 8) uint8"""
    _check_section(int(section_size))
    return (ctx or default_context()).bloombits_generate_batch(blooms, section_size)


def _kept(filters):
    """the rules NewMatcher keeps (matcher.go:105-122): none without clauses, none with a nil clause"""
    return [list(rule) for rule in filters or [] if rule and all(cl is not None for cl in rule)]


class Matcher:
    """bloombits.Matcher without its scheduler: the filter system and a match over a table"""

    def __init__(self, section_size: int, filters, ctx=None):
        self.sectionSize = int(section_size)
        self._ctx = ctx
        self._rules = _kept(filters)
        self._filters = None

    @property
    def filters(self):
        """Matcher.filters: per kept rule, the three bit numbers of each clause (calcBloomIndexes, matcher.go:
        :116), hashed on the GPU at the first read"""
        if self._filters is None:
            flat = [bytes(cl) for rule in self._rules for cl in rule]
            idx = (self._ctx or default_context()).bloom9_batch(flat).tolist() if flat else []
            it = iter(idx)
            self._filters = [[next(it) for _ in rule] for rule in self._rules]
        return self._filters

    def Matches(self, table, first_section: int, begin: int, end: int) -> np.ndarray:
        """the block numbers in [begin, end] (and inside the table) that pass the filter, ascending"""
        return MatchBatch(self.sectionSize, table, first_section, [self._rules], [begin], [end], self._ctx)[0]


def NewMatcher(section_size: int, filters, ctx=None) -> Matcher:
    _check_section(int(section_size))
    return Matcher(section_size, filters, ctx)


def MatchBatch(section_size: int, table, first_section: int, filters, begins, ends, ctx=None):
    """Many filter systems (each as NewMatcher takes one) over one table: a list of uint64 arrays"""
    _check_section(int(section_size))
    return (ctx or default_context()).bloombits_match_batch(table, section_size, first_section, filters, begins, ends)
