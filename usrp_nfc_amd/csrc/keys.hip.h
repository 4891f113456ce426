// keys.hip.h -- recovery of a MIFARE Classic sector key from ONE sniffed first authentication, stated once for host and
// device, and the three kernels that run it (k_keys_count, k_keys_fill_odd, k_keys_probe_even).  nfc_keys.hip holds the host side: the
// CPU twin (nfc_host_recover_keys), the batching and the scratch (nfc_recover_keys_device), and nfc_find_auths.
//
// Conventions are fsm.hip.h's: the 48-bit register `st`, bit i the i-th oldest bit; a clock is st = st >> 1 | nx << 47;
// the filter reads bits 9, 11, .. 47; fsmd::TAPS is the feedback.  With b_0 .. b_47 the key bits and b_{t+48} the bit shifted in at
// clock t, the clocks of a first authentication are: 0-31 uid ^ nt fed in, no keystream; 32-63 the plaintext nr fed in; 64-95 nothing
// fed, ks_t encrypts ar; 96-127 nothing fed, ks_t encrypts at.  Parity bits do not clock the register.  A 32-bit word of a frame has
// bit i = bit (i & 7) of byte (i >> 3).
//
// SPLIT.  ks_t = f(b_{t+9}, b_{t+11}, .. b_{t+47}): with O_j = b_{73+2j}, ks_{64+2k} = f(O_k .. O_{k+19}); with E_j = b_{74+2j},
// ks_{65+2k} = f(E_k .. E_{k+19}); k = 0 .. 31, j = 0 .. 50.  Per half: every 20-bit starting window that gives the first keystream
// bit is extended one bit at a time through the other 31 (walk): a 51-bit sequence per surviving path.
// JOIN.  The 54 relations b_{t+48} = xor over taps of b_{t+tap}, t = 73 .. 126, are linear: each is the xor of a mask over O and a mask
// over E.  The 54 parities of a sequence under its half's masks are its signature; a solution is a pair with equal signatures.
// Relation t + 2 is relation t moved by one place in both halves, so two base masks per half give all 54 (sig_base).
// ROLL BACK.  The pair is the register at clock 73; 73 steps back (rollback) give the register at clock 0: the key, in load_key's order.
// VERIFY.  The candidate key runs forward through fsmd's CRYPTO1 over the trace (verify): it must reproduce ar and at and decrypt {nr} to
// bytes whose four parity bits are right.
//
// NESTED.  Inside a session the tag nonce arrives encrypted, {nt}; the new sector's register is loaded with the key and
// clocked with uid ^ nt in PLAINTEXT (fsm.hip.h, the nested branch), so for ONE candidate nt a nested authentication is a first one with
// another nt.  A genuine card draws nt from a 16-bit LFSR: 65 536 candidates, a seed each (nonce_extend).  Ten ninth bits of {nt}, {ar},
// {at} are encrypted with keystream bits that follow from the candidate alone (nested_candidate): 64 seeds pass, or none.
// k_nested_candidates writes the survivors as Prepared records in ascending seed order; the three search kernels run over (nested
// trace, candidate) pairs -- virtual traces -- through an index (`map`), and verify additionally asks for ks1 and the {nt} ninth bits.
//
// READER PAIRS.  Without {at} only ks_64 .. ks_95 are known: the same walk and join at half the depth (walk<16>, a 22-bit
// signature) leave about 1e5 joined candidates, and a SECOND session of the same key decides (verify_pair).  The searches are KINDS
// (FullKind, PairKind) and the kernels templates over a kind; the pair kind's probe stages the joined registers for
// k_keys_verify_stage instead of verifying inside the walk's loop.
// NOT PROMISED: a single authentication without {at}, a nested {nt} without {at}, 7-byte UIDs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nfc_amd.h"
#include "fsm.hip.h"

namespace nfc {
namespace keys {

constexpr int N_KS = 32;                 // keystream bits per half
constexpr int WINDOW_BITS = 20;
constexpr uint32_t WINDOWS = 1u << WINDOW_BITS;
constexpr int N_REL = 54;                // relations of the join: the signature's width
constexpr uint64_t SIG_EMPTY = ~0ull;    // outside the 54-bit range
constexpr int T_JOIN = 73;               // the pair is the register at this clock

// the filter over a 20-bit window: bit i of w is register bit 9 + 2 i (fsmd::filter)
NFC_HD uint32_t filter20(uint32_t w) {
    const uint32_t a = (fsmd::TT_FA >> (w & 15u)) & 1u, b = (fsmd::TT_FB >> ((w >> 4) & 15u)) & 1u, c = (fsmd::TT_FB >> ((w >> 8) & 15u)) & 1u;
    const uint32_t d = (fsmd::TT_FA >> ((w >> 12) & 15u)) & 1u, e = (fsmd::TT_FB >> ((w >> 16) & 15u)) & 1u;
    return (fsmd::TT_FC >> (a | b << 1 | c << 2 | d << 3 | e << 4)) & 1u;
}

// Relation r (t = 73 + r) over the places j = r + tap (and r + 48, the bit shifted in): an even j is O_{j / 2}, an odd j E_{(j - 1) / 2}.
// The masks of r = 2 i + p are those of r = p shifted left by i: half 0 = O, half 1 = E.
constexpr uint64_t sig_base(int half, int p) {
    const int taps[19] = {0, 5, 9, 10, 12, 14, 15, 17, 19, 24, 25, 27, 29, 35, 39, 41, 42, 43, 48};   // fsm.hip.h: taps_mask, and the new bit
    uint64_t m = 0;
    for (int i = 0; i < 19; i++) {
        const int j = p + taps[i];
        if ((j & 1) == half) m ^= 1ull << (j >> 1);
    }
    return m;
}
constexpr uint64_t SIG_O0 = sig_base(0, 0), SIG_O1 = sig_base(0, 1), SIG_E0 = sig_base(1, 0), SIG_E1 = sig_base(1, 1);
NFC_HD uint64_t parity64(uint64_t x) { return (uint64_t)(__builtin_popcountll(x) & 1); }
template <int HALF, int NREL = N_REL>
NFC_HD uint64_t signature(uint64_t seq) {
    constexpr uint64_t B0 = HALF ? SIG_E0 : SIG_O0, B1 = HALF ? SIG_E1 : SIG_O1;
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < NREL / 2; i++) s |= parity64((seq >> i) & B0) << (2 * i) | parity64((seq >> i) & B1) << (2 * i + 1);
    return s;
}

// The extensions of one starting window, depth first and iteratively.  `seq` holds the sequence (bit j = O_j or E_j) AND the branches
// tried: at depth k the candidate bit is bit k + 19, 0 first, then 1; every bit above it is 0.  No array, so no scratch memory.
// emit(seq) sees every complete sequence (DEPTH keystream bits: 19 + DEPTH places, 51 for the full search); -> how many there were.
template <int DEPTH = N_KS, class Emit>
NFC_HD uint32_t walk(uint32_t window, uint32_t ks, Emit &&emit) {
    if (filter20(window) != (ks & 1u)) return 0u;
    uint64_t seq = window;
    int k = 1;
    uint32_t n = 0;
    for (;;) {
        if (filter20((uint32_t)(seq >> k) & (WINDOWS - 1u)) == ((ks >> k) & 1u)) {
            if (k < DEPTH - 1) {
                k++;
                continue;
            }
            emit(seq);
            n++;
        }
        while (k >= 1 && ((seq >> (k + WINDOW_BITS - 1)) & 1ull)) {   // both values tried: one level up
            seq &= ~(1ull << (k + WINDOW_BITS - 1));
            k--;
        }
        if (k == 0) break;
        seq |= 1ull << (k + WINDOW_BITS - 1);
    }
    return n;
}

// what the walk and the verification need of a trace, worked out once on the host
struct Prepared {
    uint32_t ks_odd, ks_even;   // bit k: ks_{64 + 2 k}, ks_{65 + 2 k}
    uint32_t uid_nt;            // uid ^ nt
    uint32_t nr_enc, ar_enc, at_enc;
    uint32_t ar, at;            // suc64(nt), suc96(nt)
    uint32_t par;               // the twelve parity bits as received; nested: bits 12 .. 15 those of {nt}, and PREP_NESTED
    uint32_t parent;            // nested: the index of the nested trace (0 for a first authentication)
    uint32_t nt_enc, nt;        // nested: {nt} and the candidate plaintext nonce (0 for a first authentication)
};
constexpr uint32_t PREP_NESTED = 1u << 31;
NFC_HD uint32_t even_bits(uint64_t x) {   // bits 0, 2, 4 .. 62 of x
    uint32_t r = 0;
    for (int i = 0; i < 32; i++) r |= (uint32_t)((x >> (2 * i)) & 1ull) << i;
    return r;
}
NFC_HD Prepared prepare(const nfc_auth_trace &t) {
    Prepared P;
    P.ar = fsmd::nonce_advance(t.nt, 64);
    P.at = fsmd::nonce_advance(P.ar, 32);
    const uint64_t ks = (uint64_t)(t.ar_enc ^ P.ar) | (uint64_t)(t.at_enc ^ P.at) << 32;   // ks_64 .. ks_127
    P.ks_odd = even_bits(ks);
    P.ks_even = even_bits(ks >> 1);
    P.uid_nt = t.uid ^ t.nt;
    P.nr_enc = t.nr_enc, P.ar_enc = t.ar_enc, P.at_enc = t.at_enc;
    P.par = t.par;
    P.parent = 0, P.nt_enc = 0, P.nt = 0;
    return P;
}

// ---- nested authentications: the candidate nonces ----
constexpr uint32_t NESTED_SEEDS = 1u << 16, NESTED_CANDS = 64;
// the 32 nonce bits from the first 16: b[k + 16] = b[k] ^ b[k + 2] ^ b[k + 3] ^ b[k + 5] (fsmd::nonce_advance's recurrence)
NFC_HD uint32_t nonce_extend(uint32_t seed) {
    uint32_t x = seed & 0xFFFFu;
    for (int k = 0; k < 16; k++) x |= (((x >> k) ^ (x >> (k + 2)) ^ (x >> (k + 3)) ^ (x >> (k + 5))) & 1u) << (k + 16);
    return x;
}
// a ninth bit `p` over the plaintext byte `pt`, encrypted with keystream bit `ks`: right when p ^ ks is the odd parity of pt
NFC_HD bool ninth_fits(uint32_t p, uint32_t ks, uint32_t pt) { return ((p ^ ks) & 1u) == (1u ^ (frames::popc8(pt & 0xFFu) & 1u)); }
// The record of (trace, seed), and whether the seed passes the ten tests: the ninth bit of a byte is encrypted with the keystream bit
// of the NEXT data bit, and ks1 = {nt} ^ nt, ks2 = {ar} ^ suc64(nt), ks3 = {at} ^ suc96(nt) follow from the candidate.  {nt} bytes
// 0 .. 2 with ks1 bits 8, 16, 24; {ar} bytes 0 .. 2 with ks2 bits 8, 16, 24 and byte 3 with ks3 bit 0; {at} bytes 0 .. 2 with ks3 bits
// 8, 16, 24.  (The ninth bits of {nr}, of {nt} byte 3 and of {at} byte 3 need the register or a later frame: verify's.)
NFC_HD bool nested_candidate(const nfc_nested_trace &t, uint32_t parent, uint32_t seed, Prepared &P) {
    const uint32_t nt = nonce_extend(seed);
    P.ar = fsmd::nonce_advance(nt, 64);
    P.at = fsmd::nonce_advance(P.ar, 32);
    const uint32_t ks1 = t.nt_enc ^ nt, ks2 = t.ar_enc ^ P.ar, ks3 = t.at_enc ^ P.at, par = t.par;
    bool ok = ninth_fits(par >> 7, ks3, P.ar >> 24);
    for (int b = 0; b < 3; b++) {
        ok = ok && ninth_fits(par >> (12 + b), ks1 >> (8 * b + 8), nt >> (8 * b));
        ok = ok && ninth_fits(par >> (4 + b), ks2 >> (8 * b + 8), P.ar >> (8 * b));
        ok = ok && ninth_fits(par >> (8 + b), ks3 >> (8 * b + 8), P.at >> (8 * b));
    }
    const uint64_t ks = (uint64_t)ks2 | (uint64_t)ks3 << 32;
    P.ks_odd = even_bits(ks);
    P.ks_even = even_bits(ks >> 1);
    P.uid_nt = t.uid ^ nt;
    P.nr_enc = t.nr_enc, P.ar_enc = t.ar_enc, P.at_enc = t.at_enc;
    P.par = (uint32_t)par | PREP_NESTED;
    P.parent = parent, P.nt_enc = t.nt_enc, P.nt = nt;
    return ok;
}

// the register at clock 73 from the pair: bit i = b_{73 + i}
NFC_HD uint64_t join_state(uint64_t o, uint64_t e) {
    uint64_t s = 0;
    for (int i = 0; i < 24; i++) s |= ((o >> i) & 1ull) << (2 * i) | ((e >> i) & 1ull) << (2 * i + 1);
    return s;
}
// 73 clocks back: with S' = (S << 1) & mask, b_t = S[47] ^ L(S') ^ in_t; the filter does not read bit 0, so f(S') is f(S_t)
NFC_HD uint64_t rollback(uint64_t s, const Prepared &P) {
    for (int t = T_JOIN - 1; t >= 0; t--) {
        const uint64_t sp = (s << 1) & fsmd::ST_MASK;
        const uint32_t in = t >= 64 ? 0u : t >= 32 ? (((P.nr_enc >> (t - 32)) & 1u) ^ fsmd::filter(sp)) : ((P.uid_nt >> t) & 1u);
        s = sp | (uint64_t)((((uint32_t)(s >> 47) & 1u) ^ fsmd::feedback(sp) ^ in) & 1u);
    }
    return s;
}
// the candidate key forward over the trace, as fsmd's machine runs a first authentication.  nr_out: the decrypted reader nonce.
// A nested record (PREP_NESTED) must also give ks1: over clocks 0 .. 31 the filter output xor {nt} is the candidate nt, and the four
// ninth bits of {nt} fit, each under the keystream bit of the next data bit (the fourth: clock 32, the first of {nr}).
NFC_HD bool verify(uint64_t key, const Prepared &P, uint32_t *nr_out) {
    uint64_t st = key & fsmd::ST_MASK;
    bool bad = false;
    if (P.par & PREP_NESTED) {
        uint32_t ks1 = 0;
        for (int i = 0; i < 32; i++) {
            ks1 |= fsmd::filter(st) << i;
            st = fsmd::shift_in(st, (P.uid_nt >> i) & 1u);
            if ((i & 7) == 7 && !ninth_fits(P.par >> (12 + (i >> 3)), fsmd::filter(st), P.nt >> (i - 7))) bad = true;
        }
        if ((P.nt_enc ^ ks1) != P.nt) bad = true;
    } else {
        for (int i = 0; i < 32; i++) st = fsmd::shift_in(st, (P.uid_nt >> i) & 1u);
    }
    uint32_t nr = 0;
    for (int b = 0; b < 4; b++) {
        uint32_t pt = 0;
        for (int k = 0; k < 8; k++) {
            const uint32_t f = fsmd::filter(st), bit = ((P.nr_enc >> (8 * b + k)) & 1u) ^ f;
            pt |= bit << k;
            st = fsmd::shift_in(st, bit);
        }
        // the ninth bit reuses the keystream bit of the next data bit
        if ((frames::popc8(pt) & 1u) == (((P.par >> b) & 1u) ^ fsmd::filter(st))) bad = true;
        nr |= pt << (8 * b);
    }
    uint32_t ks2 = 0, ks3 = 0;
    for (int i = 0; i < 32; i++) ks2 |= fsmd::filter(st) << i, st = fsmd::shift_in(st, 0u);
    for (int i = 0; i < 32; i++) ks3 |= fsmd::filter(st) << i, st = fsmd::shift_in(st, 0u);
    if (nr_out) *nr_out = nr;
    return !bad && (P.ar_enc ^ ks2) == P.ar && (P.at_enc ^ ks3) == P.at;
}

// ---- reader pairs: two authentications WITHOUT {at} ----
// Only ks_64 .. ks_95 are known: per half k = 0 .. 15, a 35-bit sequence, and the relations whose places all lie in the two sequences
// are t = 73 .. 94: a 22-bit signature.  About 1e5 pairs join; the register at clock 73 still needs only O_0 .. O_23 / E_0 .. E_23, so
// rollback is the full search's.  What singles the key out is a SECOND session of the same key (the check session).
constexpr int PAIR_KS = 16, PAIR_REL = 22;
struct PairRecord {
    Prepared s;   // the searched session: ks_odd / ks_even hold 16 bits each; at_enc, at 0; par: the eight ninth bits of {nr}{ar}
    uint32_t c_uid_nt, c_nr_enc, c_ar_enc, c_ar, c_par;   // the check session: uid ^ nt, {nr}, {ar}, suc64(nt), its eight ninth bits
    uint32_t pad;
};
NFC_HD PairRecord prepare_pair(const nfc_reader_pair &p) {
    PairRecord R;
    nfc_auth_trace t = p.search;
    t.at_enc = 0, t.par &= 0xFFu;
    R.s = prepare(t);
    R.s.ks_odd &= 0xFFFFu, R.s.ks_even &= 0xFFFFu;   // (the upper halves came from {at}: unknown)
    R.s.at = 0;
    R.c_uid_nt = p.check.uid ^ p.check.nt;
    R.c_nr_enc = p.check.nr_enc, R.c_ar_enc = p.check.ar_enc;
    R.c_ar = fsmd::nonce_advance(p.check.nt, 64);
    R.c_par = p.check.par & 0xFFu;
    R.pad = 0;
    return R;
}
// One reader-side session forward under `key`: {nr} decrypts to four right ninth bits, ks2 reproduces ar, and the four ninth bits of {ar}
// fit -- bytes 0 .. 2 under ks2 bits 8, 16, 24, byte 3 under ks3 bit 0 (the filter after the 32 free-running clocks).
NFC_HD bool verify_reader(uint64_t key, uint32_t uid_nt, uint32_t nr_enc, uint32_t ar_enc, uint32_t ar, uint32_t par, uint32_t *nr_out) {
    uint64_t st = key & fsmd::ST_MASK;
    for (int i = 0; i < 32; i++) st = fsmd::shift_in(st, (uid_nt >> i) & 1u);
    bool ok = true;
    uint32_t nr = 0;
    for (int b = 0; b < 4; b++) {
        uint32_t pt = 0;
        for (int k = 0; k < 8; k++) {
            const uint32_t bit = ((nr_enc >> (8 * b + k)) & 1u) ^ fsmd::filter(st);
            pt |= bit << k;
            st = fsmd::shift_in(st, bit);
        }
        ok = ok && ninth_fits(par >> b, fsmd::filter(st), pt);
        nr |= pt << (8 * b);
    }
    uint32_t ks2 = 0;
    for (int i = 0; i < 32; i++) ks2 |= fsmd::filter(st) << i, st = fsmd::shift_in(st, 0u);
    for (int b = 0; b < 3; b++) ok = ok && ninth_fits(par >> (4 + b), ks2 >> (8 * b + 8), ar >> (8 * b));
    ok = ok && ninth_fits(par >> 7, fsmd::filter(st), ar >> 24);
    if (nr_out) *nr_out = nr;
    return ok && (ar_enc ^ ks2) == ar;
}
// a joined candidate counts when it passes BOTH sessions.  nr_search / nr_check: the decrypted reader nonces (may be null)
NFC_HD bool verify_pair(uint64_t key, const PairRecord &R, uint32_t *nr_search, uint32_t *nr_check) {
    const bool a = verify_reader(key, R.s.uid_nt, R.s.nr_enc, R.s.ar_enc, R.s.ar, R.s.par, nr_search);
    if (!a && !nr_check) return false;
    const bool b = verify_reader(key, R.c_uid_nt, R.c_nr_enc, R.c_ar_enc, R.c_ar, R.c_par, nr_check);
    return a && b;
}

// The two searches as KINDS: the record, the walk's depth, the signature's width and the verification.  host_search, device_search and
// the kernels are stated once over a kind.
struct FullKind {
    using Record = Prepared;
    static constexpr int DEPTH = N_KS, NREL = N_REL;
    static constexpr bool PAIR = false;
    static NFC_HD const Prepared &base(const Record &r) { return r; }
    static NFC_HD bool check(uint64_t key, const Record &r) { return verify(key, r, nullptr); }
};
struct PairKind {
    using Record = PairRecord;
    static constexpr int DEPTH = PAIR_KS, NREL = PAIR_REL;
    static constexpr bool PAIR = true;
    static NFC_HD const Prepared &base(const Record &r) { return r.s; }
    static NFC_HD bool check(uint64_t key, const Record &r) { return verify_pair(key, r, nullptr, nullptr); }
};

// the table of a trace: a power of two, at least twice its odd list (at least 2)
inline uint32_t table_log2(uint64_t n_odd) {
    uint32_t l = 1;
    while ((1ull << l) < 2 * n_odd) l++;
    return l;
}
NFC_HD uint64_t slot_of(uint64_t sig, uint32_t log2) { return (sig * 0x9E3779B97F4A7C15ull) >> (64u - log2); }

#if defined(__HIPCC__)
// ---- the kernels.  A workgroup is 256 consecutive starting windows of one half of one trace; blockIdx.z + t0 is the trace. ----
// The trace is a place in the BATCH: counts, place, n_found and min_key are indexed by it and hold a batch's worth.  Its record is
// prep[trace], or prep[map[trace]] with a map: the virtual traces of a nested search lie where k_nested_candidates wrote them, 64
// slots per nested trace, and the host lists the batch's ones.  A record is only read, so a map entry decides what is searched and
// never where anything is written: the memory-safety argument does not depend on how many records there are.
constexpr int KEYS_BLOCK = 256;
enum { KEYS_ERR_TABLE_FULL = 1, KEYS_ERR_CANDIDATES = 2 };
template <class Record>
__device__ __forceinline__ const Record &record_of(const Record *__restrict__ prep, const uint32_t *__restrict__ map, uint32_t tr) {
    return prep[map ? map[tr] : tr];
}

// A workgroup per nested trace: NESTED_SEEDS / NESTED_BLOCK rounds of one seed per lane.  The rank of a survivor is the survivors of
// earlier rounds + those of lower waves in this round + those of lower lanes in its wave (ballot), so the order is the seeds' own and
// no atomic decides it.  Slot rank of the trace's NESTED_CANDS holds it; a rank that is not below NESTED_CANDS (it cannot be: the
// ten tests have rank 10) is not written and raises KEYS_ERR_CANDIDATES.  n_out[trace]: the survivors, at most NESTED_CANDS.
constexpr int NESTED_BLOCK = 1024, NESTED_WAVES = NESTED_BLOCK / 64;
__global__ __launch_bounds__(NESTED_BLOCK) void k_nested_candidates(const nfc_nested_trace *__restrict__ traces, Prepared *__restrict__ prep /* [trace][64] */,
                                                                    uint32_t *__restrict__ n_out, uint32_t *__restrict__ err) {
    __shared__ uint32_t wave_n[2][NESTED_WAVES];
    const uint32_t tr = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const nfc_nested_trace t = traces[tr];
    uint32_t base = 0;
    for (uint32_t round = 0; round < NESTED_SEEDS / NESTED_BLOCK; round++) {
        Prepared P;
        const bool ok = nested_candidate(t, tr, round * NESTED_BLOCK + threadIdx.x, P);
        const uint64_t votes = __ballot(ok);
        if (lane == 0) wave_n[round & 1u][wave] = (uint32_t)__popcll(votes);
        __syncthreads();   // (two buffers: a wave that runs ahead writes the other one, and meets the next barrier before this one again)
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < NESTED_WAVES; w++) {
            const uint32_t c = wave_n[round & 1u][w];
            before += w < wave ? c : 0u;
            total += c;
        }
        if (ok) {
            const uint32_t rank = base + before + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
            if (rank < NESTED_CANDS) prep[(size_t)tr * NESTED_CANDS + rank] = P;
            else atomicOr(err, (uint32_t)KEYS_ERR_CANDIDATES);
        }
        base += total;
    }
    if (threadIdx.x == 0) n_out[tr] = base < NESTED_CANDS ? base : NESTED_CANDS;
}

// per trace of the batch: where its table lies in the scratch (slots), and its size (0: the trace takes no part in this launch)
struct Place {
    uint64_t off;
    uint32_t log2, pad;
};

template <class Kind>
__global__ __launch_bounds__(KEYS_BLOCK) void k_keys_count(const typename Kind::Record *__restrict__ prep, const uint32_t *__restrict__ map,
                                                           uint32_t *__restrict__ counts /* [trace][half] */) {
    const uint32_t tr = blockIdx.z, half = blockIdx.y, w = blockIdx.x * KEYS_BLOCK + threadIdx.x;
    const uint32_t ks = half ? Kind::base(record_of(prep, map, tr)).ks_even : Kind::base(record_of(prep, map, tr)).ks_odd;
    uint32_t n = walk<Kind::DEPTH>(w, ks, [](uint64_t) {});
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    for (int off = 32; off; off >>= 1) n += __shfl_down(n, off, 64);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(&counts[2 * tr + half], total);
}

// Every slot index is masked to the trace's table, so nothing is written outside its section whatever the counts were; a table that
// turns out full (it cannot, the host sized it from the exact count) raises KEYS_ERR_TABLE_FULL and the sequence is dropped.
template <class Kind>
__global__ __launch_bounds__(KEYS_BLOCK) void k_keys_fill_odd(const typename Kind::Record *__restrict__ prep, const uint32_t *__restrict__ map,
                                                              const Place *__restrict__ place, uint32_t t0, uint64_t *__restrict__ sig_tab, uint64_t *__restrict__ seq_tab, uint32_t *__restrict__ err) {
    const uint32_t tr = t0 + blockIdx.z, w = blockIdx.x * KEYS_BLOCK + threadIdx.x;
    const Place pl = place[tr];
    if (pl.log2 == 0) return;
    const uint64_t mask = (1ull << pl.log2) - 1ull;
    walk<Kind::DEPTH>(w, Kind::base(record_of(prep, map, tr)).ks_odd, [&](uint64_t seq) {
        const uint64_t sig = signature<0, Kind::NREL>(seq);
        uint64_t slot = slot_of(sig, pl.log2);
        for (uint64_t tries = 0; tries <= mask; tries++) {
            const uint64_t old = atomicCAS((unsigned long long *)&sig_tab[pl.off + slot], (unsigned long long)SIG_EMPTY, (unsigned long long)sig);
            if (old == SIG_EMPTY) {   // equal signatures take separate slots
                seq_tab[pl.off + slot] = seq;
                return;
            }
            slot = (slot + 1) & mask;
        }
        atomicOr(err, (uint32_t)KEYS_ERR_TABLE_FULL);
    });
}

// The lanes of a wave that stand here together take consecutive places from ONE atomic of the first of them (every lane of a workgroup
// has the same trace, so the same counter) -> this lane's place.  Inside the walk's divergent loop __ballot(1) is the set of lanes
// that execute THIS call together, whichever that is; the ballot, the leader's atomic and the shuffle are straight-line code under
// one execution mask, so any such set gets distinct consecutive places (n_joined equals the twin's in the tests).
__device__ __forceinline__ uint32_t wave_append(uint32_t *counter) {
    const uint64_t here = __ballot(1);
    const uint32_t lane = threadIdx.x & 63u, first = (uint32_t)__ffsll((unsigned long long)here) - 1u;
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(counter, (uint32_t)__popcll(here));
    return (uint32_t)__shfl((int)base, (int)first, 64) + (uint32_t)__popcll(here & ((1ull << lane) - 1ull));
}
// what a verified candidate leaves: its trace's count and lowest key
template <class Kind>
__device__ __forceinline__ void settle(uint64_t joined, const typename Kind::Record &R, uint32_t *n_found, unsigned long long *min_key) {
    const uint64_t key = rollback(joined, Kind::base(R));
    if (Kind::check(key, R)) {
        atomicAdd(n_found, 1u);
        atomicMin(min_key, (unsigned long long)key);
    }
}

// STAGED false: every joined pair is rolled back and verified by the lane that found it (the full search joins about one).  STAGED
// true (reader pairs: about 1e5 join, and the 170 cipher clocks of a verification inside the walk's loop would hold a whole wave): the
// joined register goes into the trace's section of `stage`, [trace of the batch][cap] words, at the place the trace's n_joined counter
// gives, and k_keys_verify_stage settles a candidate per lane.  A place that is not below cap -- the stage is full -- is never written:
// that candidate is settled here, so nothing is truncated.  n_joined counts every equal signature (a kind that reports it: PAIR).
template <class Kind, bool STAGED>
__global__ __launch_bounds__(KEYS_BLOCK) void k_keys_probe_even(const typename Kind::Record *__restrict__ prep, const uint32_t *__restrict__ map,
                                                                const Place *__restrict__ place, uint32_t t0, const uint64_t *__restrict__ sig_tab, const uint64_t *__restrict__ seq_tab,
                                                                uint32_t *__restrict__ n_found, unsigned long long *__restrict__ min_key,
                                                                uint32_t *__restrict__ n_joined, uint64_t *__restrict__ stage, uint32_t cap) {
    const uint32_t tr = t0 + blockIdx.z, w = blockIdx.x * KEYS_BLOCK + threadIdx.x;
    const Place pl = place[tr];
    if (pl.log2 == 0) return;
    const uint64_t mask = (1ull << pl.log2) - 1ull;
    const typename Kind::Record R = record_of(prep, map, tr);
    walk<Kind::DEPTH>(w, Kind::base(R).ks_even, [&](uint64_t seq) {
        const uint64_t sig = signature<1, Kind::NREL>(seq);
        uint64_t slot = slot_of(sig, pl.log2);
        for (uint64_t tries = 0; tries <= mask; tries++) {
            const uint64_t s = sig_tab[pl.off + slot];
            if (s == SIG_EMPTY) return;
            if (s == sig) {
                const uint64_t joined = join_state(seq_tab[pl.off + slot], seq);
                if (STAGED) {
                    const uint32_t at = wave_append(&n_joined[tr]);
                    if (at < cap) stage[(size_t)tr * cap + at] = joined;
                    else settle<Kind>(joined, R, &n_found[tr], &min_key[tr]);
                } else {
                    if (Kind::PAIR) atomicAdd(&n_joined[tr], 1u);
                    settle<Kind>(joined, R, &n_found[tr], &min_key[tr]);
                }
            }
            slot = (slot + 1) & mask;
        }
    });
}

// The dense follow-up of a STAGED probe: a lane per staged candidate of the trace, min(n_joined, cap) of them, in strides of the grid.
template <class Kind>
__global__ __launch_bounds__(KEYS_BLOCK) void k_keys_verify_stage(const typename Kind::Record *__restrict__ prep, const uint32_t *__restrict__ map,
                                                                  const Place *__restrict__ place, uint32_t t0, const uint32_t *__restrict__ n_joined,
                                                                  const uint64_t *__restrict__ stage, uint32_t cap, uint32_t *__restrict__ n_found,
                                                                  unsigned long long *__restrict__ min_key) {
    const uint32_t tr = t0 + blockIdx.z;
    if (place[tr].log2 == 0) return;
    const uint32_t n = n_joined[tr] < cap ? n_joined[tr] : cap;
    if (blockIdx.x * KEYS_BLOCK >= n) return;
    const typename Kind::Record R = record_of(prep, map, tr);
    for (uint32_t i = blockIdx.x * KEYS_BLOCK + threadIdx.x; i < n; i += gridDim.x * KEYS_BLOCK)
        settle<Kind>(stage[(size_t)tr * cap + i], R, &n_found[tr], &min_key[tr]);
}
#endif   // __HIPCC__

}  // namespace keys
}  // namespace nfc
