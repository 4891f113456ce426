// keys.hip.h -- recovery of a MIFARE Classic sector key from ONE sniffed first authentication, stated once for host and
// device, and the three kernels that run it (k_keys_count, k_keys_fill_odd, k_keys_probe_even).  nfc_keys.hip holds the host side: the
// CPU twin (nfc_host_recover_keys), the batching and the scratch (nfc_recover_keys_device), and nfc_find_auths.
//
// Conventions are protocol.h's / fsm.hip.h's: the 48-bit register `st`, bit i the i-th oldest bit; a clock is st = st >> 1 | nx << 47;
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
    const int taps[19] = {0, 5, 9, 10, 12, 14, 15, 17, 19, 24, 25, 27, 29, 35, 39, 41, 42, 43, 48};   // protocol.h: Crypto1::feedback, and the new bit
    uint64_t m = 0;
    for (int i = 0; i < 19; i++) {
        const int j = p + taps[i];
        if ((j & 1) == half) m ^= 1ull << (j >> 1);
    }
    return m;
}
constexpr uint64_t SIG_O0 = sig_base(0, 0), SIG_O1 = sig_base(0, 1), SIG_E0 = sig_base(1, 0), SIG_E1 = sig_base(1, 1);
NFC_HD uint64_t parity64(uint64_t x) { return (uint64_t)(__builtin_popcountll(x) & 1); }
template <int HALF>
NFC_HD uint64_t signature(uint64_t seq) {
    constexpr uint64_t B0 = HALF ? SIG_E0 : SIG_O0, B1 = HALF ? SIG_E1 : SIG_O1;
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < N_REL / 2; i++) s |= parity64((seq >> i) & B0) << (2 * i) | parity64((seq >> i) & B1) << (2 * i + 1);
    return s;
}

// The extensions of one starting window, depth first and iteratively.  `seq` holds the sequence (bit j = O_j or E_j) AND the branches
// tried: at depth k the candidate bit is bit k + 19, 0 first, then 1; every bit above it is 0.  No array, so no scratch memory.
// emit(seq) sees every complete 51-bit sequence; -> how many there were.
template <class Emit>
NFC_HD uint32_t walk(uint32_t window, uint32_t ks, Emit &&emit) {
    if (filter20(window) != (ks & 1u)) return 0u;
    uint64_t seq = window;
    int k = 1;
    uint32_t n = 0;
    for (;;) {
        if (filter20((uint32_t)(seq >> k) & (WINDOWS - 1u)) == ((ks >> k) & 1u)) {
            if (k < N_KS - 1) {
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
    uint32_t par;               // the twelve parity bits as received
    uint32_t pad;
};
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
    P.pad = 0;
    return P;
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
NFC_HD bool verify(uint64_t key, const Prepared &P, uint32_t *nr_out) {
    uint64_t st = key & fsmd::ST_MASK;
    for (int i = 0; i < 32; i++) st = fsmd::shift_in(st, (P.uid_nt >> i) & 1u);
    uint32_t nr = 0;
    bool bad = false;
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

// the table of a trace: a power of two, at least twice its odd list (at least 2)
inline uint32_t table_log2(uint64_t n_odd) {
    uint32_t l = 1;
    while ((1ull << l) < 2 * n_odd) l++;
    return l;
}
NFC_HD uint64_t slot_of(uint64_t sig, uint32_t log2) { return (sig * 0x9E3779B97F4A7C15ull) >> (64u - log2); }

#if defined(__HIPCC__)
// ---- the kernels.  A workgroup is 256 consecutive starting windows of one half of one trace; blockIdx.z + t0 is the trace. ----
constexpr int KEYS_BLOCK = 256;
enum { KEYS_ERR_TABLE_FULL = 1 };

// per trace of the batch: where its table lies in the scratch (slots), and its size (0: the trace takes no part in this launch)
struct Place {
    uint64_t off;
    uint32_t log2, pad;
};

__global__ __launch_bounds__(KEYS_BLOCK) void k_keys_count(const Prepared *__restrict__ prep, uint32_t *__restrict__ counts /* [trace][half] */) {
    const uint32_t tr = blockIdx.z, half = blockIdx.y, w = blockIdx.x * KEYS_BLOCK + threadIdx.x;
    const uint32_t ks = half ? prep[tr].ks_even : prep[tr].ks_odd;
    uint32_t n = walk(w, ks, [](uint64_t) {});
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
__global__ __launch_bounds__(KEYS_BLOCK) void k_keys_fill_odd(const Prepared *__restrict__ prep, const Place *__restrict__ place, uint32_t t0,
                                                              uint64_t *__restrict__ sig_tab, uint64_t *__restrict__ seq_tab, uint32_t *__restrict__ err) {
    const uint32_t tr = t0 + blockIdx.z, w = blockIdx.x * KEYS_BLOCK + threadIdx.x;
    const Place pl = place[tr];
    if (pl.log2 == 0) return;
    const uint64_t mask = (1ull << pl.log2) - 1ull;
    walk(w, prep[tr].ks_odd, [&](uint64_t seq) {
        const uint64_t sig = signature<0>(seq);
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

__global__ __launch_bounds__(KEYS_BLOCK) void k_keys_probe_even(const Prepared *__restrict__ prep, const Place *__restrict__ place, uint32_t t0,
                                                                const uint64_t *__restrict__ sig_tab, const uint64_t *__restrict__ seq_tab,
                                                                uint32_t *__restrict__ n_found, unsigned long long *__restrict__ min_key) {
    const uint32_t tr = t0 + blockIdx.z, w = blockIdx.x * KEYS_BLOCK + threadIdx.x;
    const Place pl = place[tr];
    if (pl.log2 == 0) return;
    const uint64_t mask = (1ull << pl.log2) - 1ull;
    const Prepared P = prep[tr];
    walk(w, P.ks_even, [&](uint64_t seq) {
        const uint64_t sig = signature<1>(seq);
        uint64_t slot = slot_of(sig, pl.log2);
        for (uint64_t tries = 0; tries <= mask; tries++) {
            const uint64_t s = sig_tab[pl.off + slot];
            if (s == SIG_EMPTY) return;
            if (s == sig) {
                const uint64_t key = rollback(join_state(seq_tab[pl.off + slot], seq), P);
                if (verify(key, P, nullptr)) {
                    atomicAdd(&n_found[tr], 1u);
                    atomicMin(&min_key[tr], (unsigned long long)key);
                }
            }
            slot = (slot + 1) & mask;
        }
    });
}
#endif   // __HIPCC__

}  // namespace keys
}  // namespace nfc
