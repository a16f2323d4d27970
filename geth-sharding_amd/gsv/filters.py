"""eth/filters over batches, on the GPU: the bloom tests of a log filter.

    filters.New's flattening        eth/filters/filter.go:62-93
    bloomFilter                     eth/filters/filter.go:278-305

Fetching the logs of the blocks that pass, and the chain database behind Filter.Logs, stay with the caller.
"""
from __future__ import annotations

import numpy as np

from . import bloombits, default_context


def _flatten(addresses, topics):
    """filter.go:66-80: the addresses as one rule when there are any, then one rule per topic list"""
    out = []
    if addresses:
        out.append([bytes(a) for a in addresses])
    for sub in topics or []:
        out.append([bytes(t) for t in sub])
    return out


class Filter:
    """The bloom side of filters.Filter: `filters` is what New hands NewMatcher."""

    def __init__(self, addresses, topics, ctx=None):
        self.addresses = [bytes(a) for a in addresses or []]
        self.topics = [[bytes(t) for t in sub] for sub in topics or []]
        self.filters = _flatten(self.addresses, self.topics)
        self._ctx = ctx

    def Matcher(self, section_size: int) -> bloombits.Matcher:
        """the indexed part of Filter.Logs: bloombits.NewMatcher(size, filters) (filter.go:91)"""
        return bloombits.NewMatcher(section_size, self.filters, self._ctx)

    def BloomFilter(self, blooms) -> np.ndarray:
        """the unindexed tail of Filter.Logs: bloomFilter of each block's bloom (filter.go:278-305)"""
        return (self._ctx or default_context()).bloom_filter_batch(blooms, [self.filters])[0]


def BloomFilter(blooms, addresses, topics, ctx=None) -> np.ndarray:
    """bloomFilter(bloom, addresses, topics) for each bloom: (n,) bool"""
    return Filter(addresses, topics, ctx).BloomFilter(blooms)
