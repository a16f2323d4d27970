// Clique of the C ABI (include/gsv.h, "clique"): the voting snapshot and the fold of clique_host.h behind opaque
// handles.  Host only: no context, no device, no HIP call; the unit is here so that libgsv.so exports it.
#include <new>

#include "clique_host.h"

namespace cq = gsv::clique;

struct gsv_clique_snapshot {
    cq::Snapshot s;
};

namespace {

cq::Addr addr_of(const uint8_t* p) {
    cq::Addr a;
    memcpy(a.data(), p, 20);
    return a;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ the snapshot and the fold (host only)
gsv_clique_snapshot* gsv_clique_snapshot_new(const uint8_t* signers20, size_t n, uint64_t number, const uint8_t* hash32) {
    if (!hash32 || (n && !signers20)) return nullptr;
    gsv_clique_snapshot* h = new (std::nothrow) gsv_clique_snapshot();
    if (!h) return nullptr;
    h->s.number = number;
    memcpy(h->s.hash, hash32, 32);
    for (size_t i = 0; i < n; i++) h->s.signers.insert(addr_of(signers20 + 20 * i));
    return h;
}

gsv_clique_snapshot* gsv_clique_snapshot_from_genesis(const uint8_t* header_rlp, size_t len, int* status) {
    gsv_clique_snapshot* h = header_rlp ? new (std::nothrow) gsv_clique_snapshot() : nullptr;
    const uint8_t st = h ? cq::from_genesis(h->s, header_rlp, len) : (uint8_t)GSV_ST_BAD_RLP;
    if (status) *status = st;
    if (st != GSV_ST_OK) {
        delete h;
        return nullptr;
    }
    return h;
}

gsv_clique_snapshot* gsv_clique_snapshot_copy(const gsv_clique_snapshot* snap) {
    return snap ? new (std::nothrow) gsv_clique_snapshot(*snap) : nullptr;
}

void gsv_clique_snapshot_free(gsv_clique_snapshot* snap) { delete snap; }

uint64_t gsv_clique_snapshot_number(const gsv_clique_snapshot* snap) { return snap ? snap->s.number : 0; }

int gsv_clique_snapshot_hash(const gsv_clique_snapshot* snap, uint8_t* hash32) {
    if (!snap || !hash32) return GSV_E_INVALID_ARG;
    memcpy(hash32, snap->s.hash, 32);
    return GSV_SUCCESS;
}

size_t gsv_clique_snapshot_signers(const gsv_clique_snapshot* snap, uint8_t* signer20, size_t cap) {
    if (!snap) return 0;
    size_t k = 0;
    for (const cq::Addr& a : snap->s.signers) {
        if (k < cap && signer20) memcpy(signer20 + 20 * k, a.data(), 20);
        k++;
    }
    return k;
}

size_t gsv_clique_snapshot_recents(const gsv_clique_snapshot* snap, uint64_t* block, uint8_t* signer20, size_t cap) {
    if (!snap) return 0;
    size_t k = 0;
    for (const auto& kv : snap->s.recents) {
        if (k < cap) {
            if (block) block[k] = kv.first;
            if (signer20) memcpy(signer20 + 20 * k, kv.second.data(), 20);
        }
        k++;
    }
    return k;
}

size_t gsv_clique_snapshot_votes(const gsv_clique_snapshot* snap, uint8_t* signer20, uint64_t* block, uint8_t* address20,
                                 uint8_t* authorize, size_t cap) {
    if (!snap) return 0;
    size_t k = 0;
    for (const cq::Vote& v : snap->s.votes) {
        if (k < cap) {
            if (signer20) memcpy(signer20 + 20 * k, v.signer.data(), 20);
            if (block) block[k] = v.block;
            if (address20) memcpy(address20 + 20 * k, v.address.data(), 20);
            if (authorize) authorize[k] = v.authorize ? 1 : 0;
        }
        k++;
    }
    return k;
}

size_t gsv_clique_snapshot_tally(const gsv_clique_snapshot* snap, uint8_t* address20, uint8_t* authorize, int32_t* votes,
                                 size_t cap) {
    if (!snap) return 0;
    size_t k = 0;
    for (const auto& kv : snap->s.tally) {
        if (k < cap) {
            if (address20) memcpy(address20 + 20 * k, kv.first.data(), 20);
            if (authorize) authorize[k] = kv.second.authorize ? 1 : 0;
            if (votes) votes[k] = kv.second.votes;
        }
        k++;
    }
    return k;
}

int gsv_clique_snapshot_inturn(const gsv_clique_snapshot* snap, uint64_t number, const uint8_t* signer20) {
    if (!snap || !signer20) return 0;
    return cq::inturn(snap->s, number, addr_of(signer20)) ? 1 : 0;
}

int gsv_clique_calc_difficulty(const gsv_clique_snapshot* snap, const uint8_t* signer20) {
    if (!snap || !signer20) return 0;
    return cq::inturn(snap->s, snap->s.number + 1, addr_of(signer20)) ? 2 : 1;
}

int gsv_clique_fold(gsv_clique_snapshot* snap, const gsv_clique_config* config, const uint8_t* records, size_t n,
                    const uint8_t* rlp, const uint64_t* off, uint8_t* status, size_t* applied) {
    if (applied) *applied = 0;
    if (!snap || !config || config->epoch == 0) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!records || !rlp || !off || !status) return GSV_E_INVALID_ARG;
    const size_t done = cq::fold(snap->s, config->epoch, records, n, rlp, off, status);
    if (applied) *applied = done;
    return GSV_SUCCESS;
}

}  // extern "C"
