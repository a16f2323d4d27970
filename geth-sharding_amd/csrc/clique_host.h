// The host half of consensus/clique, free of HIP (plain C++17; tests/native/clique_host_main.cpp compiles it with
// g++): the fixed-width record of one header, the voting snapshot (snapshot.go) and the fold of a batch's records
// over it (what verifyCascadingFields and verifySeal do once the signer is known, clique.go:331-368, :466-503, and
// Snapshot.apply, snapshot.go:175-285).
//
// The fold is the part of Clique.VerifyHeaders that is serial by nature: a few dozen integer operations per header
// over signers already recovered (gsv_ecrecover_batch over sigHash and the seal).  It holds Signers, Recents and Tally as ordered maps (the reference's are Go maps; every place that
// reads one either looks a key up or sorts first) and Votes as the chronological list.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../../include/gsv.h"
#include "ethash_host.h"

namespace gsv {
namespace clique {

// Nonce read as a vote (clique.go:61-62)
constexpr uint32_t VOTE_DROP = 0, VOTE_AUTH = 1, VOTE_NEITHER = 2;

// ---- the record of one header, as the caller packs it for the fold: 128 bytes
//   hash 32 | parent_hash 32 | signer 20 | coinbase 20 | number 8 (little-endian) | extra_off 4 | extra_len 4 |
//   static_status 1 | signer_status 1 | vote 1 | difficulty 1 | zero 4
// extra_off: the offset of Extra's first byte from the header's first byte; extra_len: len(Extra) in full.  Both are
// zero for a header that did not decode.
constexpr size_t REC_BYTES = 128;
constexpr size_t R_HASH = 0, R_PARENT_HASH = 32, R_SIGNER = 64, R_COINBASE = 84, R_NUMBER = 104, R_EXTRA_OFF = 112,
                 R_EXTRA_LEN = 116, R_STATIC = 120, R_SIGNER_STATUS = 121, R_VOTE = 122, R_DIFFICULTY = 123;

constexpr uint32_t EXTRA_VANITY = 32, EXTRA_SEAL = 65;  // clique.go:58-59

using Addr = std::array<uint8_t, 20>;

struct Record {
    uint8_t hash[32], parent_hash[32];
    Addr signer, coinbase;
    uint64_t number;
    uint32_t extra_off, extra_len;
    uint8_t static_status, signer_status, vote, difficulty;
};

inline Record read_record(const uint8_t* p) {
    Record r;
    memcpy(r.hash, p + R_HASH, 32);
    memcpy(r.parent_hash, p + R_PARENT_HASH, 32);
    memcpy(r.signer.data(), p + R_SIGNER, 20);
    memcpy(r.coinbase.data(), p + R_COINBASE, 20);
    r.number = 0;
    for (int k = 7; k >= 0; k--) r.number = r.number << 8 | p[R_NUMBER + k];
    r.extra_off = (uint32_t)p[R_EXTRA_OFF] | (uint32_t)p[R_EXTRA_OFF + 1] << 8 | (uint32_t)p[R_EXTRA_OFF + 2] << 16 |
                  (uint32_t)p[R_EXTRA_OFF + 3] << 24;
    r.extra_len = (uint32_t)p[R_EXTRA_LEN] | (uint32_t)p[R_EXTRA_LEN + 1] << 8 | (uint32_t)p[R_EXTRA_LEN + 2] << 16 |
                  (uint32_t)p[R_EXTRA_LEN + 3] << 24;
    r.static_status = p[R_STATIC];
    r.signer_status = p[R_SIGNER_STATUS];
    r.vote = p[R_VOTE];
    r.difficulty = p[R_DIFFICULTY];
    return r;
}

inline void write_record(uint8_t* p, const Record& r) {
    memset(p, 0, REC_BYTES);
    memcpy(p + R_HASH, r.hash, 32);
    memcpy(p + R_PARENT_HASH, r.parent_hash, 32);
    memcpy(p + R_SIGNER, r.signer.data(), 20);
    memcpy(p + R_COINBASE, r.coinbase.data(), 20);
    for (int k = 0; k < 8; k++) p[R_NUMBER + k] = (uint8_t)(r.number >> (8 * k));
    for (int k = 0; k < 4; k++) p[R_EXTRA_OFF + k] = (uint8_t)(r.extra_off >> (8 * k));
    for (int k = 0; k < 4; k++) p[R_EXTRA_LEN + k] = (uint8_t)(r.extra_len >> (8 * k));
    p[R_STATIC] = r.static_status;
    p[R_SIGNER_STATUS] = r.signer_status;
    p[R_VOTE] = r.vote;
    p[R_DIFFICULTY] = r.difficulty;
}

// ---- the snapshot (snapshot.go:30-57)
struct Vote {
    Addr signer;
    uint64_t block;
    Addr address;
    bool authorize;
};

struct Tally {
    bool authorize;
    int votes;
};

struct Snapshot {
    uint64_t number = 0;
    uint8_t hash[32] = {0};
    std::set<Addr> signers;            // ascending, as Snapshot.signers() sorts them (snapshot.go:288-301)
    std::map<uint64_t, Addr> recents;
    std::vector<Vote> votes;           // chronological
    std::map<Addr, Tally> tally;
};

// cast / uncast (snapshot.go:131-171)
inline bool cast(Snapshot& s, const Addr& address, bool authorize) {
    const bool signer = s.signers.count(address) != 0;
    if (!((signer && !authorize) || (!signer && authorize))) return false;
    auto it = s.tally.find(address);
    if (it != s.tally.end()) it->second.votes++;
    else s.tally[address] = Tally{authorize, 1};
    return true;
}

inline bool uncast(Snapshot& s, const Addr& address, bool authorize) {
    auto it = s.tally.find(address);
    if (it == s.tally.end()) return false;
    if (it->second.authorize != authorize) return false;
    if (it->second.votes > 1) it->second.votes--;
    else s.tally.erase(it);
    return true;
}

// Snapshot.inturn (snapshot.go:304-310); false for an empty signer set, where the reference divides by zero
inline bool inturn(const Snapshot& s, uint64_t number, const Addr& signer) {
    if (s.signers.empty()) return false;
    uint64_t offset = 0;
    for (const Addr& a : s.signers) {
        if (a == signer) break;
        offset++;
    }
    return number % (uint64_t)s.signers.size() == offset;
}

// One header of Snapshot.apply (snapshot.go:192-280) over its record, GSV_ST_OK or the failure.  Every test that
// can fail comes before the first change, so a failing header leaves the snapshot as it was (the reference
// discards its copy).  OURS: a header that did not decode, or whose ParentHash is not the snapshot's Hash, is
// GSV_ST_UNKNOWN_ANCESTOR (the reference's snapshot() would walk to its database, clique.go:408-425).
inline uint8_t apply_one(Snapshot& s, uint64_t epoch, const Record& r) {
    if (r.static_status == GSV_ST_BAD_RLP || r.static_status == GSV_ST_HEADER_TOO_WIDE) return GSV_ST_UNKNOWN_ANCESTOR;
    if (memcmp(s.hash, r.parent_hash, 32) != 0) return GSV_ST_UNKNOWN_ANCESTOR;
    if (r.number != s.number + 1) return GSV_ST_CLIQUE_VOTING_CHAIN;  // :181-188
    const uint64_t number = r.number;
    const uint64_t limit = (uint64_t)s.signers.size() / 2 + 1;
    const bool drop = number >= limit;  // :200-202, the oldest recent signer may sign again
    if (r.signer_status != GSV_ST_OK) return r.signer_status;  // :204-207
    if (!s.signers.count(r.signer)) return GSV_ST_CLIQUE_UNAUTHORIZED;
    for (const auto& kv : s.recents)
        if (kv.second == r.signer && !(drop && kv.first == number - limit)) return GSV_ST_CLIQUE_UNAUTHORIZED;
    if (r.vote != VOTE_AUTH && r.vote != VOTE_DROP) return GSV_ST_CLIQUE_INVALID_VOTE;  // :231-238
    // from here on nothing fails
    if (number % epoch == 0) {  // :195-198
        s.votes.clear();
        s.tally.clear();
    }
    if (drop) s.recents.erase(number - limit);
    s.recents[number] = r.signer;
    for (size_t i = 0; i < s.votes.size(); i++) {  // :219-228
        if (s.votes[i].signer == r.signer && s.votes[i].address == r.coinbase) {
            uncast(s, s.votes[i].address, s.votes[i].authorize);
            s.votes.erase(s.votes.begin() + (ptrdiff_t)i);
            break;
        }
    }
    const bool authorize = r.vote == VOTE_AUTH;
    if (cast(s, r.coinbase, authorize)) s.votes.push_back(Vote{r.signer, number, r.coinbase, authorize});
    auto it = s.tally.find(r.coinbase);  // :248-279
    if (it != s.tally.end() && it->second.votes > (int)(s.signers.size() / 2)) {
        if (it->second.authorize) {
            s.signers.insert(r.coinbase);
        } else {
            s.signers.erase(r.coinbase);
            const uint64_t lim2 = (uint64_t)s.signers.size() / 2 + 1;
            if (number >= lim2) s.recents.erase(number - lim2);
            for (size_t i = 0; i < s.votes.size();) {
                if (s.votes[i].signer == r.coinbase) {
                    uncast(s, s.votes[i].address, s.votes[i].authorize);
                    s.votes.erase(s.votes.begin() + (ptrdiff_t)i);
                } else {
                    i++;
                }
            }
        }
        for (size_t i = 0; i < s.votes.size();) {
            if (s.votes[i].address == r.coinbase) s.votes.erase(s.votes.begin() + (ptrdiff_t)i);
            else i++;
        }
        s.tally.erase(r.coinbase);
    }
    s.number = number;
    memcpy(s.hash, r.hash, 32);
    return GSV_ST_OK;
}

// verifySeal behind the recovery (clique.go:478-502) over the snapshot at the header's parent
inline uint8_t verify_seal(const Snapshot& s, const Record& r) {
    if (r.signer_status != GSV_ST_OK) return r.signer_status;
    if (!s.signers.count(r.signer)) return GSV_ST_CLIQUE_UNAUTHORIZED;
    const uint64_t limit = (uint64_t)s.signers.size() / 2 + 1;
    for (const auto& kv : s.recents)
        if (kv.second == r.signer && kv.first > r.number - limit) return GSV_ST_CLIQUE_UNAUTHORIZED;  // uint64, as Go's
    const bool turn = inturn(s, r.number, r.signer);
    if (turn && r.difficulty != 2) return GSV_ST_CLIQUE_DIFFICULTY;
    if (!turn && r.difficulty != 1) return GSV_ST_CLIQUE_DIFFICULTY;
    return GSV_ST_OK;
}

// The fold of include/gsv.h's gsv_clique_fold.  records: n x REC_BYTES; rlp / off: the caller's headers on the host
// (read only for a checkpoint's signer list, at the record's offsets).  Returns the number of headers applied.
inline size_t fold(Snapshot& s, uint64_t epoch, const uint8_t* records, size_t n, const uint8_t* rlp,
                   const uint64_t* off, uint8_t* status) {
    uint8_t err = GSV_ST_OK;
    size_t applied = 0;
    for (size_t i = 0; i < n; i++) {
        const Record r = read_record(records + i * REC_BYTES);
        uint8_t st = r.static_status;
        if (st == GSV_ST_OK && r.number != 0) {
            if (err != GSV_ST_OK) {
                st = err;  // snapshot() failed on an earlier header (:351-354)
            } else {
                if (r.number % epoch == 0) {  // :356-365
                    const size_t want = s.signers.size() * 20;
                    bool same = (size_t)r.extra_len == want + EXTRA_VANITY + EXTRA_SEAL;
                    if (same) {
                        const uint8_t* p = rlp + off[i] + r.extra_off + EXTRA_VANITY;
                        size_t k = 0;
                        for (const Addr& a : s.signers) same = same && memcmp(p + 20 * k++, a.data(), 20) == 0;
                    }
                    if (!same) st = GSV_ST_CLIQUE_CHECKPOINT_SIGNERS;
                }
                if (st == GSV_ST_OK) st = verify_seal(s, r);
            }
        }
        status[i] = st;
        // the header becomes a parent of the next one whatever its own verdict (the reference applies a parent that
        // failed verifyHeader, too); the genesis header is never applied (:334)
        const bool genesis = r.static_status != GSV_ST_BAD_RLP && r.static_status != GSV_ST_HEADER_TOO_WIDE && r.number == 0;
        if (err == GSV_ST_OK && !genesis) {
            err = apply_one(s, epoch, r);
            if (err == GSV_ST_OK) applied++;
        }
    }
    return applied;
}

// ---- the genesis snapshot (clique.go:392-401): the signer list of Extra[32 : len - 65] of an RLP-encoded header.
// A host walk over the list's 15 strings by the encoder's rules (shortest lengths, no item past the list).
inline bool host_rlp_string(const uint8_t* p, size_t& pos, size_t end, size_t& off, size_t& len) {
    if (pos >= end) return false;
    const uint32_t b = p[pos];
    if (b < 0x80u) {
        off = pos, len = 1, pos += 1;
        return true;
    }
    if (b <= 0xB7u) {
        len = b - 0x80u, off = pos + 1;
        if (len > end - off || (len == 1 && p[off] < 0x80u)) return false;
        pos = off + len;
        return true;
    }
    if (b > 0xBFu) return false;
    const size_t ll = b - 0xB7u;
    if (ll > 4 || ll > end - (pos + 1)) return false;
    size_t size = 0;
    for (size_t k = 0; k < ll; k++) size = size << 8 | p[pos + 1 + k];
    if (p[pos + 1] == 0 || size < 56) return false;
    off = pos + 1 + ll;
    if (size > end - off) return false;
    len = size, pos = off + size;
    return true;
}

// GSV_ST_OK and the snapshot at block 0, or GSV_ST_BAD_RLP / GSV_ST_CLIQUE_MISSING_VANITY / _MISSING_SIGNATURE
inline uint8_t from_genesis(Snapshot& s, const uint8_t* rlp, size_t len) {
    static const size_t fixed[15] = {32, 32, 20, 32, 32, 32, 256, 0, 0, 0, 0, 0, 0, 32, 8};
    if (len == 0 || len > 0xFFFFFFFFull || rlp[0] < 0xC0u) return GSV_ST_BAD_RLP;
    size_t head = 1, payload = rlp[0] - 0xC0u;
    if (rlp[0] > 0xF7u) {
        const size_t ll = rlp[0] - 0xF7u;
        if (ll > 4 || 1 + ll > len) return GSV_ST_BAD_RLP;
        payload = 0;
        for (size_t k = 0; k < ll; k++) payload = payload << 8 | rlp[1 + k];
        if (rlp[1] == 0 || payload < 56) return GSV_ST_BAD_RLP;
        head = 1 + ll;
    }
    if (payload != len - head) return GSV_ST_BAD_RLP;
    size_t pos = head, off = 0, n = 0, extra_off = 0, extra_len = 0;
    for (int f = 0; f < 15; f++) {
        if (!host_rlp_string(rlp, pos, len, off, n)) return GSV_ST_BAD_RLP;
        if (fixed[f] && n != fixed[f]) return GSV_ST_BAD_RLP;
        if (f == 12) extra_off = off, extra_len = n;
    }
    if (pos != len) return GSV_ST_BAD_RLP;
    if (extra_len < EXTRA_VANITY) return GSV_ST_CLIQUE_MISSING_VANITY;
    if (extra_len < EXTRA_VANITY + EXTRA_SEAL) return GSV_ST_CLIQUE_MISSING_SIGNATURE;
    s = Snapshot();
    const size_t count = (extra_len - EXTRA_VANITY - EXTRA_SEAL) / 20;
    for (size_t i = 0; i < count; i++) {
        Addr a;
        memcpy(a.data(), rlp + extra_off + EXTRA_VANITY + 20 * i, 20);
        s.signers.insert(a);
    }
    gsv::ethash::keccak256(s.hash, rlp, len);
    return GSV_ST_OK;
}

}  // namespace clique
}  // namespace gsv
