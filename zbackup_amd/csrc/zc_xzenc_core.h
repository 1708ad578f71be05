// xz / LZMA2 / LZMA encoding for the write path, written for host and device
// alike (ZC_HD, as zc_xz_core.h): the GPU bundle encoder (zc_xzenc.hip) runs
// exactly what the CPU unit check (tests/xzenc/xzenc_core_check.cpp) holds to
// liblzma's decoder, and the host gives the device's bytes.
//
// What zbackup writes: Bundle::Creator compresses a bundle's payload with
// lzma_easy_encoder(6, LZMA_CHECK_CRC64) (compression.cc:78-97).  An xz stream
// is defined by its decoder, so the bytes here are not liblzma's: any stream
// that lzma_stream_decoder and zc_xz_core.h read back to the payload is a
// valid bundle body.  Written from the xz file format (1.0.4) and the LZMA2 /
// LZMA descriptions, not from a library; the probability layout and the CRC
// code are zc_xz_core.h's.
//
// The stream: one block, its only filter LZMA2, check id 0, 1 or 4, the
// properties fixed at lc=3, lp=0, pb=2, the dictionary property the smallest
// LZMA2 size that covers the payload (4 KiB at least), a block header without
// size fields (as liblzma's easy encoder writes it).  An empty payload gives
// the 32-byte stream without a block.
//
// LZMA2 chunks: chunk k covers payload bytes [64 Ki * k, 64 Ki * (k + 1)), so
// the stored form can always take a chunk's place.  A chunk is coded in its
// LZMA form behind space left for its header (6 bytes with properties, 5
// without); its compressed size c is known at every step as a lower bound
// (bytes written + bytes the range coder holds back + 4), and the moment
// header + c >= 3 + payload the LZMA form is given up and the chunk written
// stored over it (control 1 for the stream's first chunk, 2 afterwards).  That
// is also the rule that keeps c within the 16-bit size field: c < payload <=
// 64 Ki for every kept chunk.  The LZMA chunk after a stored one resets the
// state (0xA0, or 0xC0 with the properties if none were sent yet), so no
// probability is ever rolled back.  The stream's first chunk, when LZMA, is
// 0xE0; the dictionary is reset only there (control 0xE0 or 1), so every
// earlier payload byte stays reachable.
//
// Match finding is a pure function of the payload (pick() below): positions in
// groups of 64; position p's table candidate is the latest position with the
// same hash of its 4 bytes among the groups before p's own, from a table whose
// update is a maximum; distances 1 .. 64 are tried directly on top (they cover
// p's own group).  The candidate array (a distance and a length up to 64 per
// position, 0: none) is the encoder's input; the four rep distances are tried
// by the parse itself.
//
// The parse is greedy: the longest rep match if it is long enough, else the
// candidate, else a short rep or a literal.  One step of laziness (a literal
// when the next position's candidate is longer) measured larger on the CPU
// (2 MiB text-like 446,544 against 444,452 bytes, four-letter 674,012 against
// 654,700), so there is none.
//
//   in.byte(i)                  payload byte, i < n: the walk asks for p and p - 1
//   in.back_byte(i)             the same for a byte anywhere behind p
//   in.word(i)                  bytes i .. i + 3, little-endian, i + 4 <= n
//   in.match_len(p, d, limit)   the count of k < limit, from 0 up, with
//                               byte(p + k) == byte(p + k - d); 1 <= d <= p, p + limit <= n
//   in.rep_lens(p, d, limit, l) l[r] = match_len(p, d[r], limit), 0 where d[r] > p
//   in.cand(p)                  the candidate of position p as pick() packs it (0: none)
//   probs.ld / st / fill        as zc_xz_core.h
//   out.put(pos, b)             stream[pos] = b, pos < cap (checked here first)
//   out.stored(pos, src, len)   stream[pos + k] = payload[src + k], checked first
//   out.finish()                once, after the last put: a sink may hold bytes back until then
//
// Termination: one loop; a trip opens a chunk, closes one or codes a symbol of
// at least one payload byte, so n + 2 * chunks + 8 trips, fixed before the
// walk, bound it.  Every match comparison is bounded by the chunk's end, which
// is at most the payload's.  The range coder's pending-byte loop is bounded by
// the bytes of the chunk.  No goto.
#pragma once
#include <stdint.h>

#include "zc_xz_core.h"

namespace zcxzenc {

using namespace zcxz;

constexpr uint64_t kMaxPayload = 64ull << 20;
constexpr uint32_t kChunk = 65536;
constexpr uint32_t kLc = 3, kLp = 0, kPb = 2;
constexpr uint32_t kPropsByte = (kPb * 5 + kLp) * 9 + kLc;  // 0x5D
constexpr uint32_t kHashBits = 17;                          // the table: 2^17 entries of 8 bytes
constexpr uint32_t kNear = 64;                              // distances tried directly
constexpr uint32_t kNice = 64;                              // pick() compares no further

// the symbol kinds a check program may count
enum Kind {
  kKLiteral = 0, kKMatchedLiteral, kKMatch, kKShortRep, kKRep0, kKRep1, kKRep2, kKRep3, kKLenLow, kKLenMid, kKLenHigh,
  kKDistSlotOnly, kKDistSpecial, kKDistDirect, kKStored, kKLzmaChunk, kKinds
};
struct NoCount {
  ZC_XZ_FN void hit(int) {}
};

// container + 3 bytes per 64 KiB + payload: header 12, block header 12, end byte and
// block padding 4, check 8, index 16, footer 12
ZC_XZ_FN uint64_t capacity(uint64_t n) { return n == 0 ? 32 : n + 3 * ((n + kChunk - 1) / kChunk) + 64; }

// the smallest LZMA2 dictionary property whose size covers n (4 KiB at least)
ZC_XZ_FN uint32_t dict_prop_for(uint64_t n) {
  uint32_t prop = 0;
  for (uint32_t k = 0; k < 40 && (uint64_t)dict_size_of(prop) < n; ++k) ++prop;
  return prop;
}

ZC_XZ_FN uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - kHashBits); }

// A candidate as the array holds it: (length - 1) << 26 | distance - 1, 0: none.
// The length is 4 .. kNice, measured up to the payload's end, and kNice stands for
// "kNice or more"; the distance is below 2^26 = kMaxPayload.
constexpr uint32_t kCandDistBits = 26;
static_assert(kMaxPayload <= (1ull << kCandDistBits) && kNice - 1 < (1u << (32 - kCandDistBits)), "a candidate's fields");

// The candidate of position p; p + 4 <= n.  t1 is 1 + the table's position for
// hash4(word(p)), 0 when it has none; the table holds positions of groups
// before p's own only, so t1 - 1 < p.  Lengths are compared up to kNice bytes.
template <class In>
ZC_XZ_FN uint32_t pick(const In& in, uint64_t n, uint64_t p, uint64_t t1) {
  const uint32_t w = in.word(p);
  const uint32_t maxlen = n - p < kNice ? (uint32_t)(n - p) : kNice;
  const uint32_t near = p < kNear ? (uint32_t)p : kNear;
  uint32_t best_len = 0, best_d = 0;
  for (uint32_t d = 1; d <= near && best_len < maxlen; ++d) {
    if (in.word(p - d) == w) {
      const uint32_t l = 4 + in.match_len(p + 4, d, maxlen - 4);
      if (l > best_len) {
        best_len = l;
        best_d = d;
      }
    }
  }
  if (t1 != 0 && t1 - 1 < p && best_len < maxlen) {
    const uint64_t t = t1 - 1;
    const uint32_t d = (uint32_t)(p - t);
    if (in.word(t) == w) {
      const uint32_t l = 4 + in.match_len(p + 4, d, maxlen - 4);
      // a farther match has to be longer; one byte longer only if it is not 128 times as far
      if (best_len == 0 || l > best_len + 1 || (l == best_len + 1 && (d >> 7) <= best_d)) {
        best_len = l;
        best_d = d;
      }
    }
  }
  return best_len == 0 ? 0 : (best_len - 1) << kCandDistBits | (best_d - 1);
}

// The range coder: carries go through a cache byte and a count of pending 0xFF bytes.
template <class Probs, class Out>
struct Rc {
  Probs* probs;
  Out* out;
  uint64_t low, pending;  // pending: the cache byte and the 0xFF bytes behind it
  uint32_t range, cache;
  uint64_t pos, cap;  // the next stream byte; stores at pos >= cap are dropped and remembered
  bool over;

  ZC_XZ_FN void put(uint32_t b) {
    if (pos < cap)
      out->put(pos, b & 0xff);
    else
      over = true;
    ++pos;
  }
  ZC_XZ_FN void put_at(uint64_t at, uint32_t b) {
    if (at < cap)
      out->put(at, b & 0xff);
    else
      over = true;
  }
  ZC_XZ_FN void start() {
    low = 0;
    pending = 1;
    range = 0xffffffffu;
    cache = 0;
  }
  ZC_XZ_FN void shift_low() {
    if ((uint32_t)low < 0xff000000u || (low >> 32) != 0) {
      const uint32_t carry = (uint32_t)(low >> 32);
      put(cache + carry);
      for (; pending > 1; --pending) put(0xff + carry);  // at most the chunk's bytes
      pending = 0;
      cache = (uint32_t)(low >> 24) & 0xff;
    }
    ++pending;
    low = (low & 0x00ffffffu) << 8;
  }
  ZC_XZ_FN void flush() {
    for (int k = 0; k < 5; ++k) shift_low();
  }
  // n <= 16 modeled bits of one symbol at once: coded bit k is bit k of `bits`, its
  // probability idx_of(k); the probabilities of a batch are distinct (a path down a tree,
  // flags of different arrays).  The encoder knows a symbol before it codes it, so the
  // probabilities are read and updated together (probs.gather_update: a lane each on the
  // device) and only the range / low recurrence below is serial.  Probs::kBatched false:
  // the plain form, a probability read and written per bit.
  template <class F>
  ZC_XZ_FN void batch(uint32_t n, uint32_t bits, F idx_of) {
    if (Probs::kBatched) {
      const typename Probs::Vec pv = probs->gather_update(n, bits, idx_of);
      for (uint32_t k = 0; k < n; ++k) step(probs->vec_get(pv, k), (bits >> k) & 1);
    } else {
      for (uint32_t k = 0; k < n; ++k) {
        const uint32_t i = idx_of(k), p = probs->ld(i), b = (bits >> k) & 1;
        probs->st(i, b ? p - (p >> 5) : p + ((2048 - p) >> 5));
        step(p, b);
      }
    }
  }
  ZC_XZ_FN void step(uint32_t p, uint32_t b) {
    const uint32_t bound = (range >> 11) * p;
    if (b == 0) {
      range = bound;
    } else {
      low += bound;
      range -= bound;
    }
    if (range < (1u << 24)) {  // bound >= 2^13 and range - bound >= 2^13: one shift suffices
      range <<= 8;
      shift_low();
    }
  }
  // up to four flags of different arrays
  ZC_XZ_FN void flags(uint32_t n, uint32_t bits, uint32_t i0, uint32_t i1, uint32_t i2, uint32_t i3) {
    batch(n, bits, [=](uint32_t k) { return k == 0 ? i0 : k == 1 ? i1 : k == 2 ? i2 : i3; });
  }
  // the first `bits` bits of v from the top, as a batch's mask (coded bit k = bit bits - 1 - k of v)
  ZC_XZ_FN static uint32_t msb_first(uint32_t v, uint32_t bits) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < 8; ++k)
      if (k < bits) m |= ((v >> (bits - 1 - k)) & 1) << k;
    return m;
  }
  // `nf` <= 2 flags f0, f1 (values in the low bits of fbits), then v down the tree of `bits` <= 8 bits at base
  ZC_XZ_FN void flags_tree(uint32_t nf, uint32_t fbits, uint32_t f0, uint32_t f1, uint32_t base, uint32_t bits,
                           uint32_t v) {
    batch(nf + bits, fbits | msb_first(v, bits) << nf, [=](uint32_t k) {
      const uint32_t j = k < nf ? 0 : k - nf;  // the tree's step
      return k < nf ? (k == 0 ? f0 : f1) : base + ((1u << j) | (v >> (bits - j)));
    });
  }
  ZC_XZ_FN void tree(uint32_t base, uint32_t bits, uint32_t v) { flags_tree(0, 0, 0, 0, base, bits, v); }
  ZC_XZ_FN void tree_reverse(uint32_t base, uint32_t bits, uint32_t v) {  // bits <= 5
    batch(bits, v & ((1u << bits) - 1), [=](uint32_t k) {
      uint32_t r = 0;  // the low k bits of v, the lowest on top
      for (uint32_t j = 0; j < 5; ++j)
        if (j < k) r = (r << 1) | ((v >> j) & 1);
      return base + ((1u << k) | r);
    });
  }
  ZC_XZ_FN void direct(uint32_t v, uint32_t bits) {
    for (uint32_t k = bits; k > 0; --k) {
      range >>= 1;
      if ((v >> (k - 1)) & 1) low += range;
      if (range < (1u << 24)) {
        range <<= 8;
        shift_low();
      }
    }
  }
  template <class Count>
  ZC_XZ_FN void length(uint32_t base, uint32_t pos_state, uint32_t len, Count& cnt) {
    const uint32_t l = len - 2;
    if (l < 8) {
      flags_tree(1, 0, base + kLenChoice, 0, base + kLenLow + pos_state * 8, 3, l);
      cnt.hit(kKLenLow);
    } else if (l < 16) {
      flags_tree(2, 1, base + kLenChoice, base + kLenChoice2, base + kLenMid + pos_state * 8, 3, l - 8);
      cnt.hit(kKLenMid);
    } else {
      flags_tree(2, 3, base + kLenChoice, base + kLenChoice2, base + kLenHigh, 8, l - 16);
      cnt.hit(kKLenHigh);
    }
  }
};

struct EncResult {
  int status;        // kOk or kOutput
  uint32_t stored;   // chunks written in the stored form
  uint64_t size;     // the stream's length (status kOk)
};

ZC_XZ_FN uint32_t top_bit(uint32_t v) {  // v > 0
  uint32_t k = 0;
  for (uint32_t s = 16; s > 0; s >>= 1)
    if (v >> (k + s)) k += s;
  return k;
}

// Encodes the payload in[0, n), n <= kMaxPayload, whose check under check_id is
// check_value (check_of on the host, the check kernel on the device), into a
// stream of at most cap bytes.
template <class In, class Probs, class Out, class Count>
ZC_XZ_FN EncResult encode(const In& in, const uint64_t n, const uint64_t cap, const uint32_t check_id,
                          const uint64_t check_value, Probs& probs, Out& out, Count& cnt) {
  EncResult r{kOk, 0, 0};
  Rc<Probs, Out> z;
  z.probs = &probs;
  z.out = &out;
  z.pos = 0;
  z.cap = cap;
  z.over = false;
  z.start();
  // ---- stream header: FD 37 7A 58 5A 00, two flag bytes, CRC32 ----
  for (uint32_t k = 0; k < 6; ++k) z.put(magic_byte(k));
  z.put(0);
  z.put(check_id);
  const uint32_t flags_crc = ~crc32_byte(crc32_byte(0xffffffffu, 0), check_id);
  for (uint32_t k = 0; k < 4; ++k) z.put(flags_crc >> (8 * k));
  uint64_t unpadded = 0;
  if (n > 0) {
    // ---- block header: size, flags, filter id, property size, dictionary, padding, CRC32 ----
    const uint32_t bh[8] = {2, 0, 0x21, 1, dict_prop_for(n), 0, 0, 0};
    uint32_t c = 0xffffffffu;
    for (uint32_t k = 0; k < 8; ++k) {
      z.put(bh[k]);
      c = crc32_byte(c, bh[k]);
    }
    c = ~c;
    for (uint32_t k = 0; k < 4; ++k) z.put(c >> (8 * k));
    const uint64_t data_start = z.pos;

    // ---- LZMA2 ----
    uint32_t state = 0, reps[4] = {0, 0, 0, 0};
    bool first = true, props_sent = false, need_reset = true, in_chunk = false, running = true, trial_failed = false;
    uint64_t p = 0, cs = 0, ce = 0, hdr_pos = 0;
    uint32_t hdr_len = 0;
    uint64_t budget = n + 2 * ((n + kChunk - 1) / kChunk) + 8;
    for (; budget > 0 && running; --budget) {
      if (z.over) {
        // Room ran out.  Inside a chunk's LZMA form the stored form may still fit (when the
        // LZMA form would have been kept it is the smaller one, and the stored form runs out
        // of room as well): try that once, so the outcome never depends on the capacity.
        if (in_chunk && !trial_failed) {
          z.over = false;
          trial_failed = true;
        } else {
          running = false;
          continue;
        }
      }
      if (!in_chunk) {
        if (p >= n) {
          running = false;
          continue;
        }
        cs = p;
        ce = n - p < kChunk ? n : p + kChunk;
        hdr_len = props_sent ? 5 : 6;
        hdr_pos = z.pos;
        z.pos += hdr_len;
        if (need_reset) {
          probs.fill(kProbsCommon);
          state = 0;
          reps[0] = reps[1] = reps[2] = reps[3] = 0;
        }
        z.start();
        in_chunk = true;
        trial_failed = false;
        continue;
      }
      const uint64_t u = ce - cs;
      const uint64_t c_low = z.pos - (hdr_pos + hdr_len) + z.pending + 4;  // what the chunk's LZMA form takes at least
      const bool give_up = trial_failed || hdr_len + c_low >= 3 + u;
      if (p == ce || give_up) {
        // ---- the chunk's end ----
        bool lzma = !give_up;
        uint64_t c = 0;
        if (lzma) {
          z.flush();
          c = z.pos - (hdr_pos + hdr_len);
          lzma = hdr_len + c < 3 + u;
        }
        if (lzma) {
          const uint32_t ctl = first ? 0xE0 : !props_sent ? 0xC0 : need_reset ? 0xA0 : 0x80;
          z.put_at(hdr_pos, ctl | (uint32_t)((u - 1) >> 16));
          z.put_at(hdr_pos + 1, (uint32_t)((u - 1) >> 8));
          z.put_at(hdr_pos + 2, (uint32_t)(u - 1));
          z.put_at(hdr_pos + 3, (uint32_t)((c - 1) >> 8));
          z.put_at(hdr_pos + 4, (uint32_t)(c - 1));
          if (hdr_len == 6) z.put_at(hdr_pos + 5, kPropsByte);
          props_sent = true;
          need_reset = false;
          cnt.hit(kKLzmaChunk);
        } else {
          z.pos = hdr_pos;
          z.put(first ? 1 : 2);
          z.put((uint32_t)((u - 1) >> 8));
          z.put((uint32_t)(u - 1));
          if (z.pos <= cap && cap - z.pos >= u)
            out.stored(z.pos, cs, (uint32_t)u);
          else
            z.over = true;
          z.pos += u;
          need_reset = true;
          r.stored += 1;
          cnt.hit(kKStored);
        }
        first = false;
        p = ce;
        in_chunk = false;
        continue;
      }
      // ---- one symbol at p < ce ----
      const uint32_t limit = ce - p < kMatchLenMax ? (uint32_t)(ce - p) : kMatchLenMax;
      const uint32_t pos_state = (uint32_t)p & ((1u << kPb) - 1);
      const uint32_t rd[4] = {reps[0] + 1, reps[1] + 1, reps[2] + 1, reps[3] + 1};
      uint32_t rl[4];
      in.rep_lens(p, rd, limit, rl);
      uint32_t ri = 0;
      for (uint32_t k = 1; k < 4; ++k)
        if (rl[k] > rl[ri]) ri = k;
      const uint32_t rep_len = rl[ri];
      // the candidate: its length is the finder's, cut at the chunk's end, and measured on
      // only where the finder stopped at kNice
      const uint32_t ce32 = in.cand(p);
      uint32_t cd = 0, cl = 0;
      if ((ce32 >> kCandDistBits) != 0) {
        const uint32_t d = (ce32 & ((1u << kCandDistBits) - 1)) + 1, l = (ce32 >> kCandDistBits) + 1;
        if ((uint64_t)d <= p) {
          cd = d;
          cl = l < limit ? l : limit;
          if (l >= kNice && limit > kNice) cl = kNice + in.match_len(p + kNice, d, limit - kNice);
        }
      }
      if (cl < 3 || (cl == 3 && cd > 4096)) cl = 0;  // a new distance costs more than the literals it saves
      // a rep match costs no distance: it wins unless the candidate is longer by more the farther it is
      const bool use_rep = rep_len >= 2 && (rep_len + 1 >= cl || (rep_len + 2 >= cl && cd >= (1u << 9)) ||
                                            (rep_len + 3 >= cl && cd >= (1u << 15)));
      const uint32_t im = kIsMatch + state * kPosStatesMax + pos_state;
      if (use_rep) {
        // is_match 1, is_rep 1, then rep0: 0 and "long" 1; rep1: 1 0; rep2: 1 1 0; rep3: 1 1 1
        if (ri == 0) {
          z.flags(4, 0xB, im, kIsRep + state, kIsRep0 + state, kIsRep0Long + state * kPosStatesMax + pos_state);
        } else {
          if (ri == 1) {
            z.flags(4, 0x7, im, kIsRep + state, kIsRep0 + state, kIsRep1 + state);
          } else {
            z.flags(4, 0xF, im, kIsRep + state, kIsRep0 + state, kIsRep1 + state);
            z.flags(1, ri - 2, kIsRep2 + state, 0, 0, 0);
          }
          const uint32_t d = reps[ri];
          for (uint32_t k = ri; k > 0; --k) reps[k] = reps[k - 1];
          reps[0] = d;
        }
        z.length(kRepLen, pos_state, rep_len, cnt);
        state = state < 7 ? 8 : 11;
        cnt.hit(kKRep0 + (int)ri);
        p += rep_len;
      } else if (cl != 0) {
        z.flags(2, 1, im, kIsRep + state, 0, 0);
        z.length(kMatchLen, pos_state, cl, cnt);
        const uint32_t d = cd - 1;
        uint32_t slot = d;
        if (d >= 4) {
          const uint32_t nb = top_bit(d);
          slot = 2 * nb + ((d >> (nb - 1)) & 1);
        }
        z.tree(kDistSlot + (cl < 6 ? cl - 2 : 3) * 64, 6, slot);
        if (slot >= 4) {
          const uint32_t nbits = (slot >> 1) - 1;
          const uint32_t base = (2 | (slot & 1)) << nbits;
          const uint32_t rest = d - base;
          if (slot < 14) {
            z.tree_reverse(kDistSpecial + base - slot - 1, nbits, rest);
            cnt.hit(kKDistSpecial);
          } else {
            z.direct(rest >> 4, nbits - 4);
            z.tree_reverse(kDistAlign, 4, rest & 15);
            cnt.hit(kKDistDirect);
          }
        } else {
          cnt.hit(kKDistSlotOnly);
        }
        reps[3] = reps[2];
        reps[2] = reps[1];
        reps[1] = reps[0];
        reps[0] = d;
        state = state < 7 ? 7 : 10;
        cnt.hit(kKMatch);
        p += cl;
      } else if (rl[0] >= 1) {
        // a short rep: the byte at the last distance
        z.flags(4, 0x3, im, kIsRep + state, kIsRep0 + state, kIsRep0Long + state * kPosStatesMax + pos_state);
        state = state < 7 ? 9 : 11;
        cnt.hit(kKShortRep);
        p += 1;
      } else {
        // is_match 0, then the byte's eight bits from the top down its tree
        const uint32_t lit = in.byte(p);
        const uint32_t prev = p > 0 ? in.byte(p - 1) : 0;  // the dictionary is reset at 0 only
        const uint32_t base = kLiteral + 0x300u * (prev >> (8 - kLc));
        const uint32_t mask = z.msb_first(lit, 8) << 1;
        if (state < 7) {
          z.batch(9, mask, [=](uint32_t k) {
            const uint32_t j = k == 0 ? 0 : k - 1;
            return k == 0 ? im : base + ((1u << j) | (lit >> (8 - j)));
          });
          cnt.hit(kKLiteral);
        } else {
          // after a match: the byte at the last distance steers the tree for as long as the
          // literal's bits equal its bits; a match was coded since the last state reset, so
          // reps[0] < p
          const uint32_t mb = (uint64_t)reps[0] < p ? in.back_byte(p - reps[0] - 1) : 0;
          z.batch(9, mask, [=](uint32_t k) {
            const uint32_t j = k == 0 ? 0 : k - 1;
            const bool steer = (lit >> (8 - j)) == (mb >> (8 - j));  // the j bits so far are the match byte's
            const uint32_t off = steer ? 0x100u + (((mb >> (7 - j)) & 1) << 8) : 0;
            return k == 0 ? im : base + off + ((1u << j) | (lit >> (8 - j)));
          });
          cnt.hit(kKMatchedLiteral);
        }
        state = state < 4 ? 0 : state < 10 ? state - 3 : state - 6;
        p += 1;
      }
    }
    if (!z.over && (in_chunk || p != n)) z.over = true;  // the trip count ran out: never, by the count above
    // ---- end byte, block padding, check ----
    z.put(0);
    const uint64_t csize = z.pos - data_start;
    for (uint32_t k = 0; k < 3 && (z.pos - data_start) % 4 != 0; ++k) z.put(0);
    const uint32_t csz = check_size(check_id);
    for (uint32_t k = 0; k < csz; ++k) z.put((uint32_t)(check_value >> (8 * k)));
    unpadded = 12 + csize + csz;
  }
  // ---- index: 00, the record count, the record, padding, CRC32 ----
  const uint64_t xstart = z.pos;
  uint32_t c = 0xffffffffu;
  z.put(0);
  c = crc32_byte(c, 0);
  z.put(n > 0 ? 1 : 0);
  c = crc32_byte(c, n > 0 ? 1 : 0);
  if (n > 0) {
    const uint64_t vals[2] = {unpadded, n};
    for (uint32_t f = 0; f < 2; ++f) {
      uint64_t v = vals[f];
      bool more = true;
      for (uint32_t k = 0; k < 9 && more; ++k) {
        const uint32_t b = (uint32_t)(v & 0x7f) | (v >= 0x80 ? 0x80 : 0);
        z.put(b);
        c = crc32_byte(c, b);
        v >>= 7;
        more = v != 0;
      }
    }
  }
  for (uint32_t k = 0; k < 3 && (z.pos - xstart) % 4 != 0; ++k) {
    z.put(0);
    c = crc32_byte(c, 0);
  }
  c = ~c;
  for (uint32_t k = 0; k < 4; ++k) z.put(c >> (8 * k));
  // ---- stream footer: CRC32, backward size, flags, 'Y' 'Z' ----
  const uint32_t back = (uint32_t)((z.pos - xstart) / 4 - 1);
  const uint32_t tail[6] = {back & 0xff, (back >> 8) & 0xff, (back >> 16) & 0xff, back >> 24, 0, check_id};
  c = 0xffffffffu;
  for (uint32_t k = 0; k < 6; ++k) c = crc32_byte(c, tail[k]);
  c = ~c;
  for (uint32_t k = 0; k < 4; ++k) z.put(c >> (8 * k));
  for (uint32_t k = 0; k < 6; ++k) z.put(tail[k]);
  z.put(0x59);
  z.put(0x5A);
  out.finish();
  if (z.over) {
    r.status = kOutput;
    r.size = 0;
  } else {
    r.size = z.pos;
  }
  return r;
}

// ---- the host's match finder: the table as the device keeps it, a maximum per entry ----

// cand[p] for every p < n from in; table: 2^kHashBits entries, zero on entry
template <class In>
inline void find_all(const In& in, uint64_t n, uint64_t* table, uint32_t* cand) {
  for (uint64_t g = 0; g < n; g += 64) {
    const uint64_t ge = n - g < 64 ? n : g + 64;
    for (uint64_t p = g; p < ge; ++p) cand[p] = p + 4 <= n ? pick(in, n, p, table[hash4(in.word(p))]) : 0;
    for (uint64_t p = g; p < ge; ++p) {
      if (p + 4 <= n) {
        uint64_t* e = &table[hash4(in.word(p))];
        if (*e < p + 1) *e = p + 1;
      }
    }
  }
}

}  // namespace zcxzenc
