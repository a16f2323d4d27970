"""GPU parity of gsv_collation_header_verify_batch and its _dev form (csrc/collation.hip) with the CPU
oracle over the corpus of tests/header_cases.py: every RLP length of the header (73..189 bytes signed,
6..123 unsigned: both Keccak blocks, the pad byte at 135 / 136 / 137, both list-header forms, integers of
every byte length), every nil-flag combination and every status, at every position of a 256-lane
workgroup.  hash32, signer and status are compared byte for byte."""
import random

import numpy as np
import pytest

import header_cases as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(oracle):
    return H.corpus(oracle)


@pytest.fixture(scope="module")
def shuffled(cases):
    """the corpus in a seeded shuffle: neighbouring lanes of k_header_hash's [word][lane] LDS array hold
    preimages of different lengths"""
    order = list(cases)
    random.Random(1234).shuffle(order)
    return order


def _run(ctx, cases):
    return ctx.collation_header_verify_batch(*H.pack(cases))


def _check(cases, h, signer, st, what):
    """h / signer / st (any of them None: not produced) against each case's expected results"""
    bad = []
    for i, c in enumerate(cases):
        got = [h is None or bytes(h[i]) == c.hash32, signer is None or bytes(signer[i]) == c.signer,
               st is None or int(st[i]) == c.status]
        if not all(got):
            wrong = [name for name, ok in zip(("hash32", "signer", "status"), got) if not ok]
            bad.append(f"[{i}] {c.label}: rlp {len(c.rlp)} B (unsigned {len(c.unsigned_rlp)} B), nil bits {c.nil}, "
                       f"wrong {'/'.join(wrong)}" + ("" if st is None else f", status {int(st[i])} want {c.status}"))
    assert not bad, f"{what}: {len(bad)} of {len(cases)} cases disagree with the oracle\n" + "\n".join(bad[:8])


def test_whole_corpus_host_path(ctx, cases):
    _check(cases, *_run(ctx, cases), "corpus in order")


def test_whole_corpus_shuffled(ctx, shuffled):
    _check(shuffled, *_run(ctx, shuffled), "corpus shuffled")


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_prefixes_around_one_workgroup(ctx, shuffled, n):
    _check(shuffled[:n], *_run(ctx, shuffled[:n]), f"first {n} of the shuffled corpus")


def test_sampled_cases_alone(ctx, cases):
    # a batch of one: lane 0 of a workgroup whose other lanes leave at once
    for c in random.Random(99).sample(cases, 32):
        _check([c], *_run(ctx, [c]), "alone")


def test_result_ignores_the_bytes_of_a_nil_signature_row(ctx, cases, oracle):
    # the same unsigned header over three fillings of its sig65 row, next to its validly signed form
    d = [c for c in cases if c.family == "d" and c.nil & 4]
    assert len({c.sig_row for c in d}) == 4  # two valid signatures, zeros, 0xA5
    rc, _ = oracle.ecrecover(d[0].msg, d[0].sig_row)
    assert rc == 1  # left in the row, it would recover
    h, signer, st = _run(ctx, d)
    _check(d, h, signer, st, "nil signature")
    assert (st == H.ST_INVALID_SIG_LEN).all() and not signer.any()
    assert len({bytes(x) for x in h[:3]}) == 1 and bytes(h[0]) == d[0].msg


@pytest.mark.parametrize("want_hash,want_signer", [(True, True), (False, True), (True, False), (False, False)])
def test_dev_path_optional_outputs(ctx, shuffled, want_hash, want_signer):
    import torch
    n = 257
    d = [c for c in shuffled if c.family == "d"]
    part = d + [c for c in shuffled if c.family != "d"][:n - len(d)]  # every status among mixed lengths
    random.Random(5).shuffle(part)
    assert len(part) == n and len({c.nil for c in part}) == 8 and {c.status for c in part} == H.ALL_STATUSES
    host = _run(ctx, part)
    _check(part, *host, "host path of the slice")
    dev = [torch.from_numpy(a).cuda() for a in H.pack(part)]
    h = torch.full((n + 1, 32), 0xEE, dtype=torch.uint8, device="cuda") if want_hash else None
    signer = torch.full((n + 1, 20), 0xEE, dtype=torch.uint8, device="cuda") if want_signer else None
    st = torch.full((n + 1,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the fills ran on torch's stream, the call runs on the context's
    ctx.collation_header_verify_batch_dev(*dev[:5], st, nil_t=dev[5], hash_t=h, signer_t=signer)
    torch.cuda.synchronize()
    h, signer, st = (None if t is None else t.cpu().numpy() for t in (h, signer, st))
    for t, ref in zip((h, signer, st), host):
        if t is not None:
            assert (t[n:] == 0xEE).all(), "row past n written"
            assert t[:n].tobytes() == ref.tobytes()
    _check(part, None if h is None else h[:n], None if signer is None else signer[:n], st[:n], "_dev path")
