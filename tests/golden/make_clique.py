"""Writes tests/golden/clique.json: the scenarios of the reference's TestVoting (consensus/clique/snapshot_test.go:93-330)
transcribed as data (epoch, signer names, votes, expected names), and the plan of a valid 64-header chain (epoch 8,
period 1, five signers, in-turn and out-of-turn difficulties, one signer voted in and one voted out) with the values
the model (tests/clique_model.py) gives for it.  Accounts are names; a name's key is clique_model.key_of(name).

    python tests/golden/make_clique.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import block_header_model as B  # noqa: E402
import clique_model as M  # noqa: E402


def V(signer, voted=None, auth=False):
    d = {"signer": signer}
    if voted is not None:
        d.update(voted=voted, auth=auth)
    return d


# snapshot_test.go:93-330, in order
VOTING = [
    dict(epoch=0, signers=["A"], votes=[V("A")], results=["A"]),
    dict(epoch=0, signers=["A"], votes=[V("A", "B", True), V("B"), V("A", "C", True)], results=["A", "B"]),
    dict(epoch=0, signers=["A", "B"],
         votes=[V("A", "C", True), V("B", "C", True), V("A", "D", True), V("B", "D", True), V("C"), V("A", "E", True),
                V("B", "E", True)], results=["A", "B", "C", "D"]),
    dict(epoch=0, signers=["A"], votes=[V("A", "A", False)], results=[]),
    dict(epoch=0, signers=["A", "B"], votes=[V("A", "B", False)], results=["A", "B"]),
    dict(epoch=0, signers=["A", "B"], votes=[V("A", "B", False), V("B", "B", False)], results=["A"]),
    dict(epoch=0, signers=["A", "B", "C"], votes=[V("A", "C", False), V("B", "C", False)], results=["A", "B"]),
    dict(epoch=0, signers=["A", "B", "C", "D"], votes=[V("A", "C", False), V("B", "C", False)],
         results=["A", "B", "C", "D"]),
    dict(epoch=0, signers=["A", "B", "C", "D"], votes=[V("A", "D", False), V("B", "D", False), V("C", "D", False)],
         results=["A", "B", "C"]),
    dict(epoch=0, signers=["A", "B"], votes=[V("A", "C", True), V("B"), V("A", "C", True), V("B"), V("A", "C", True)],
         results=["A", "B"]),
    dict(epoch=0, signers=["A", "B"],
         votes=[V("A", "C", True), V("B"), V("A", "D", True), V("B"), V("A"), V("B", "D", True), V("A"),
                V("B", "C", True)], results=["A", "B", "C", "D"]),
    dict(epoch=0, signers=["A", "B"], votes=[V("A", "B", False), V("B"), V("A", "B", False), V("B"), V("A", "B", False)],
         results=["A", "B"]),
    dict(epoch=0, signers=["A", "B", "C", "D"],
         votes=[V("A", "C", False), V("B"), V("C"), V("A", "D", False), V("B"), V("C"), V("A"), V("B", "D", False),
                V("C", "D", False), V("A"), V("B", "C", False)], results=["A", "B"]),
    dict(epoch=0, signers=["A", "B", "C"],
         votes=[V("C", "B", False), V("A", "C", False), V("B", "C", False), V("A", "B", False)], results=["A", "B"]),
    dict(epoch=0, signers=["A", "B", "C"],
         votes=[V("C", "B", False), V("A", "C", False), V("B", "C", False), V("A", "B", False)], results=["A", "B"]),
    dict(epoch=0, signers=["A", "B", "C", "D"],
         votes=[V("A", "C", False), V("B"), V("C"), V("A", "D", False), V("B", "C", False), V("C"), V("A"),
                V("B", "D", False), V("C", "D", False)], results=["A", "B", "C"]),
    dict(epoch=0, signers=["A", "B", "C", "D"],
         votes=[V("A", "C", False), V("B"), V("C"), V("A", "D", False), V("B", "C", False), V("C"), V("A"),
                V("B", "D", False), V("C", "D", False), V("A"), V("C", "C", True)], results=["A", "B"]),
    dict(epoch=0, signers=["A", "B", "C", "D"],
         votes=[V("A", "C", False), V("B"), V("C"), V("A", "D", False), V("B", "C", False), V("C"), V("A"),
                V("B", "D", False), V("C", "D", False), V("A"), V("B", "C", True)], results=["A", "B", "C"]),
    dict(epoch=0, signers=["A", "B", "C", "D", "E"],
         votes=[V("A", "F", True), V("B", "F", True), V("C", "F", True), V("D", "F", False), V("E", "F", False),
                V("B", "F", False), V("C", "F", False), V("D", "F", True), V("E", "F", True), V("B", "A", False),
                V("C", "A", False), V("D", "A", False), V("B", "F", True)], results=["B", "C", "D", "E", "F"]),
    dict(epoch=3, signers=["A", "B"], votes=[V("A", "C", True), V("B"), V("A"), V("B", "C", True)], results=["A", "B"]),
]

CHAIN_EPOCH, CHAIN_PERIOD, CHAIN_LEN = 8, 1, 64
CHAIN_SIGNERS = ["A", "B", "C", "D", "E"]
# block -> (voted, auth): F voted in by three of five, then B voted out by four of six
CHAIN_VOTES = {2: ("F", True), 3: ("F", True), 4: ("F", True), 18: ("B", False), 19: ("B", False), 20: ("B", False),
               21: ("B", False)}


def chain_plan():
    """The signer of each block by the model: the in-turn signer when it may sign, every fifth block (and whenever
    the in-turn one is recent) the first other signer that may; a voting block is signed by someone who has not yet
    cast that vote."""
    names = {M.address(M.key_of(n)): n for n in "ABCDEF"}
    genesis = B.encode_header(M.genesis_header([M.address(M.key_of(n)) for n in CHAIN_SIGNERS]))
    snap = M.Snapshot([M.address(M.key_of(n)) for n in CHAIN_SIGNERS], 0, B.header_hash(genesis))
    plan, t = [], B.decode_header(genesis)["Time"]
    for number in range(1, CHAIN_LEN + 1):
        limit = len(snap.Signers) // 2 + 1
        recent = {s for b, s in snap.Recents.items() if b > number - limit}
        order = snap.signers()
        turn = order[number % len(order)]
        vote = CHAIN_VOTES.get(number)
        voted_by = {v["Signer"] for v in snap.Votes if vote and v["Address"] == M.address(M.key_of(vote[0]))}
        ok = [s for s in order if s not in recent and s not in voted_by and
              not (vote and s == M.address(M.key_of(vote[0])))]
        pick = turn if turn in ok and number % 5 else next(s for s in ok if s != turn)
        step = {"signer": names[pick]}
        if vote:
            step.update(voted=vote[0], auth=vote[1])
        plan.append(step)
        _, snap = M.chain_step(snap, step, t, CHAIN_EPOCH, CHAIN_PERIOD)
        t += CHAIN_PERIOD
    return plan


def main():
    plan = chain_plan()
    signers = [M.address(M.key_of(n)) for n in CHAIN_SIGNERS]
    genesis = B.encode_header(M.genesis_header(signers))
    blobs, snaps = M.build_chain(plan, signers, CHAIN_EPOCH, CHAIN_PERIOD, genesis)
    diffs = [B.decode_header(b)["Difficulty"] for b in blobs]
    assert 1 in diffs and 2 in diffs
    names = {M.address(M.key_of(n)): n for n in "ABCDEF"}
    out = {
        "accounts": {n: {"key": M.key_of(n).hex(), "address": M.address(M.key_of(n)).hex()} for n in ["", *"ABCDEF"]},
        "voting": VOTING,
        "chain": {"epoch": CHAIN_EPOCH, "period": CHAIN_PERIOD, "signers": CHAIN_SIGNERS, "plan": plan,
                  "genesis": genesis.hex(), "difficulties": diffs, "last_hash": B.header_hash(blobs[-1]).hex(),
                  "final_signers": sorted(names[a] for a in snaps[-1].Signers)},
    }
    with open(os.path.join(HERE, "clique.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
