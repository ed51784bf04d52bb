// JPEG ingest, entropy = sync: a self-synchronising parallel Huffman decoder after Klein & Wiseman and Weissenberger &
// Schmidt, stated once for the kernels (jpeg_decode_kernels.hip) and their host twin.  A restart segment is decoded by many lanes.
//
//   positions    A segment's bytes [begin, end) of the stuffed stream are cut into subsequences of S bytes; Q consecutive subsequences of
//                one segment are a sequence (one workgroup).  A position is (byte, bit) relative to the segment's begin: the data byte
//                that holds the next unread bit, and the bit 0 .. 7 in it.  It never points at a stuffing 00: behind the last bit of an FF
//                data byte it is (byte + 2, 0).  Behind `end` the bytes are zero and positions keep counting.
//   state        (position, j, k) at a symbol boundary: j the block within the MCU, k the zigzag index of the next coefficient (0: a DC
//                symbol comes next).
//   walk         decodes symbols while the position is in front of the subsequence's end: the symbol that straddles the end belongs to
//                the subsequence.  -> the exit state and the number of blocks completed.  What the sequential routine calls an error (a
//                16-bit code that matches nothing, a run or a ZRL that leaves the block) ends the block: k = 0, j = (j + 1) % bpm, one
//                more block completed, the position behind the bits consumed (a code not found consumes 16).
//   round 0      lane i walks from the guess (start of i, 0, 0) -> X[i]; for a segment's first subsequence the guess is the truth.
//   local rounds per sequence: every lane whose predecessor's X changed in the round before walks again from X[i - 1]; at most Q rounds.
//   global rounds per frame, one lane per sequence: a lane whose predecessor sequence's last X changed walks its sequence from the front
//                until an exit equals the stored one; if it rewrites its last X the next sequence is marked.  In the first round every
//                sequence but a segment's first is marked: its first subsequence has only been walked from the guess so far.  At most as many rounds as the frame has sequences.  After round r the first r sequences of a
//                segment are final, so the states are the sequential decoder's for any bytes.
//   block index  B[i], the block in progress at the entry of i: the segment's first block plus the exclusive sum of the completed blocks.
//   write pass   one lane per subsequence walks from X[i - 1] with B[i]; non-zero AC coefficients go to coef[B][k], the DC DIFFERENCE to
//                coef[B][0]; it stops at its end or when B reaches the segment's block count.  The segment's last subsequence has no end:
//                its lane goes on over zero bits until the count is reached, as the sequential routine does.
//   status       the minimum over (subsequence << 3 | code): codes 1 and 2 from the subsequence that meets them on the true path, 3 and 4
//                from the one in which the segment's last block ends -- the sequential routine's first error.
//   DC pass      per segment and component an inclusive sum of the DC differences in scan order, modulo 2^16.
// Every loop is bounded by what is named above; no lane waits for another workgroup.
#pragma once
#include "jpeg_decode.h"

namespace mi355 {

constexpr uint32_t kJpegSyncNoEnd = 0xFFFFFFFFu;

// a 64-bit window like JpegBits that also keeps the exact position of the next unread bit
template <class Fetch>
struct JpegPosBits {
    Fetch f, g;                                 // f fills the window, g steps the position
    uint32_t base, len;                         // the segment's begin within the scan, its length
    uint32_t byte = 0, bit = 0, rb = 0;
    unsigned long long win = 0; int n = 0;
    MI355_HD unsigned data(Fetch& x, uint32_t i) { return i < len ? x.at(base + i) : 0u; }
    MI355_HD void seek(uint32_t by, uint32_t bi) {
        byte = rb = by; bit = 0; win = 0; n = 0;
        fill();
        win <<= bi; n -= (int)bi; bit = bi;
    }
    MI355_HD void fill() {
        while (n <= 56) {
            const unsigned b = data(f, rb);
            rb += b == 0xFFu ? 2u : 1u;
            win |= (unsigned long long)b << (56 - n);
            n += 8;
        }
    }
    MI355_HD unsigned peek(int l) const { return (unsigned)(win >> (64 - l)); }
    MI355_HD void drop(int l) {
        win <<= l; n -= l; bit += (uint32_t)l;
        while (bit >= 8u) { bit -= 8u; byte += data(g, byte) == 0xFFu ? 2u : 1u; }
    }
    // the position of the first whole data byte at or behind the current one
    MI355_HD uint32_t next_whole() { return bit ? byte + (data(g, byte) == 0xFFu ? 2u : 1u) : byte; }
};

// the write pass's side of a walk
struct JpegSyncWrite {
    int16_t* coef;
    uint32_t B, count;                          // the block in progress; the segment's first block + its blocks
    int err;                                    // the first of kJpegDecCodeNotFound / kJpegDecRunPastBlock met
};

// walk: from `in` while the position is in front of byte `end` of the segment (kJpegSyncNoEnd: until w->B reaches w->count).
// w == nullptr: a speculative walk, nothing is stored.  `last`: the position at the exit, for the status of the segment's end.
template <class Fetch>
MI355_HD JpegSyncState jpeg_sync_walk(const JpegDecFrame& f, const JpegHuff* huff, Fetch fetch, uint32_t begin, uint32_t len, uint32_t end,
                                      JpegSyncState in, uint32_t& ends, JpegSyncWrite* w, JpegPosBits<Fetch>* last) {
    JpegPosBits<Fetch> b{fetch, fetch, begin, len};
    b.seek(in.byte, in.meta & 7u);
    int j = (int)((in.meta >> 3) & 7u), k = (int)(in.meta >> 6);
    const int ny = f.ncomp == 1 ? 1 : f.hs * f.vs;
    ends = 0;
    while (b.byte < end) {
        if (w && w->B >= w->count) break;
        const int c = j < ny ? 0 : j - ny + 1;
        bool done = false;
        int err = 0;
        b.fill();
        if (k == 0) {
            const int s = jpeg_dec_symbol(b, huff[f.dc_tab[c]]);
            if (s < 0) { b.drop(16); err = kJpegDecCodeNotFound; done = true; }
            else {
                const int v = jpeg_dec_receive(b, s & 15);
                if (w && v) w->coef[(size_t)w->B * 64] = (int16_t)v;
                k = 1;
            }
        } else {
            int s = jpeg_dec_symbol(b, huff[2 + f.ac_tab[c]]);
            if (s < 0) { b.drop(16); err = kJpegDecCodeNotFound; done = true; }
            else {
                const int r = s >> 4;
                s &= 15;
                if (!s) {
                    if (r != 15) done = true;                            // EOB
                    else { k += 16; if (k > 64) err = kJpegDecRunPastBlock; if (k >= 64) done = true; }
                } else {
                    k += r;
                    if (k > 63) { err = kJpegDecRunPastBlock; done = true; }
                    else {
                        const int v = jpeg_dec_receive(b, s);
                        if (w && v) w->coef[(size_t)w->B * 64 + k] = (int16_t)v;
                        if (++k == 64) done = true;
                    }
                }
            }
        }
        if (done) {
            k = 0; j = j + 1 == f.bpm ? 0 : j + 1; ++ends;
            if (w) { ++w->B; if (err && !w->err) w->err = err; }
        }
    }
    if (last) *last = b;
    return JpegSyncState{b.byte, b.bit | (uint32_t)j << 3 | (uint32_t)k << 6};
}

// the guess of round 0: the subsequence's first byte, or the one behind it when that is a stuffing zero
template <class Fetch>
MI355_HD JpegSyncState jpeg_sync_guess(Fetch& fetch, uint32_t begin, uint32_t li, int S) {
    uint32_t by = li * (uint32_t)S;
    if (li && fetch.at(begin + by - 1) == 0xFFu) ++by;
    return JpegSyncState{by, 0u};
}
// the end of subsequence li for the speculative rounds
MI355_HD uint32_t jpeg_sync_end(uint32_t li, int S, uint32_t len) { const uint32_t e = (li + 1) * (uint32_t)S; return e < len ? e : len; }

// the status of a segment from the walk in which its last block ended: 0, kJpegDecSegmentShort or kJpegDecSegmentLong
template <class Fetch>
MI355_HD int jpeg_sync_end_status(JpegPosBits<Fetch>& b) {
    if (((unsigned long long)b.byte << 3 | b.bit) > (unsigned long long)b.len << 3) return kJpegDecSegmentShort;
    if (b.next_whole() < b.len) return kJpegDecSegmentLong;
    return kJpegDecOk;
}

// one lane of the write pass: subsequence t of sequence q.  -> the status key, 0xFFFFFFFF when the lane has nothing to report
template <class Fetch>
MI355_HD uint32_t jpeg_sync_write_lane(const JpegDecFrame& f, const JpegHuff* huff, Fetch fetch, const JpegSyncSeg& sg, const JpegSyncSeq& sq,
                                       uint32_t t, JpegSyncState in, uint32_t B) {
    const uint32_t li = sq.lsub0 + t, count = sg.blk0 + sg.nblk;
    if (B >= count) return 0xFFFFFFFFu;
    JpegSyncWrite w{f.coef, B, count, 0};
    JpegPosBits<Fetch> last{fetch, fetch, 0, 0};
    uint32_t ends;
    jpeg_sync_walk(f, huff, fetch, sg.begin, sg.len, li + 1 == sg.nsub ? kJpegSyncNoEnd : (li + 1) * (uint32_t)f.sy.S, in, ends, &w, &last);
    int code = w.err;
    if (!code && w.B >= count) code = jpeg_sync_end_status(last);
    return code ? (sq.sub0 + t) << 3 | (uint32_t)code : 0xFFFFFFFFu;
}

// the blocks of component c in scan order: element e of the frame -> block, and whether a segment starts there
MI355_HD long long jpeg_sync_dc_count(const JpegDecFrame& f, int c) {
    const int ny = f.ncomp == 1 ? 1 : f.hs * f.vs;
    return (long long)f.mcus_x * f.mcus_y * (c ? 1 : ny);
}
MI355_HD long long jpeg_sync_dc_block(const JpegDecFrame& f, int c, long long e, bool& first) {
    const int ny = f.ncomp == 1 ? 1 : f.hs * f.vs;
    const long long mcu = c ? e : e / ny;
    const int jj = c ? 0 : (int)(e - mcu * ny);
    first = jj == 0 && mcu % f.seg_mcus == 0;
    return mcu * f.bpm + (c ? ny + c - 1 : jj);
}

// ---- tables ------------------------------------------------------------------------------------------------------------------------------
struct JpegSyncTables {
    std::vector<JpegSyncSeg> segs;
    std::vector<JpegSyncSeq> seqs;
    uint32_t nsub = 0;
};
inline void jpeg_sync_tables(const JpegParsed& P, int S, int Q, JpegSyncTables& T) {
    const JpegDecFrame& f = P.f;
    const long long mcus = (long long)f.mcus_x * f.mcus_y;
    T.segs.resize((size_t)f.nseg); T.seqs.clear(); T.nsub = 0;
    for (int s = 0; s < f.nseg; ++s) {
        JpegSyncSeg& g = T.segs[(size_t)s];
        const long long mcu0 = (long long)s * f.seg_mcus, nm = mcus - mcu0 < f.seg_mcus ? mcus - mcu0 : f.seg_mcus;
        g.begin = P.seg[2 * (size_t)s]; g.len = P.seg[2 * (size_t)s + 1] - g.begin;
        g.blk0 = (uint32_t)(mcu0 * f.bpm); g.nblk = (uint32_t)(nm * f.bpm);
        g.sub0 = T.nsub; g.nsub = g.len ? (g.len + (uint32_t)S - 1) / (uint32_t)S : 1u;
        g.seq0 = (uint32_t)T.seqs.size(); g.nseq = (g.nsub + (uint32_t)Q - 1) / (uint32_t)Q;
        for (uint32_t q = 0; q < g.nseq; ++q)
            T.seqs.push_back(JpegSyncSeq{(uint32_t)s, g.sub0 + q * (uint32_t)Q, g.nsub - q * (uint32_t)Q < (uint32_t)Q ? g.nsub - q * (uint32_t)Q : (uint32_t)Q, q * (uint32_t)Q});
        T.nsub += g.nsub;
    }
}

// ---- host twin: the kernels' rounds, executed synchronously --------------------------------------------------------------------------------
// coef (jpeg_dec_blocks x 64, zeroed here) -> status.  states (or NULL): nsub entry states; stats (or NULL)
inline int jpeg_sync_coefficients_host(const JpegParsed& P, const uint8_t* data, int S, int Q, int16_t* coef, mi355_jpeg_sync_state* states,
                                       mi355_jpeg_sync_stats* stats) {
    JpegDecFrame f = P.f;
    f.coef = coef; f.sy.S = S; f.sy.Q = Q;
    std::memset(coef, 0, (size_t)jpeg_dec_blocks(f) * 128);
    JpegSyncTables T;
    jpeg_sync_tables(P, S, Q, T);
    const uint32_t nsub = T.nsub, nseq = (uint32_t)T.seqs.size();
    JpegFetchBytes fetch{data + P.scan_begin};
    std::vector<JpegSyncState> X(nsub), nx(nsub);
    std::vector<uint32_t> E(nsub), B(nsub);
    std::vector<uint8_t> chg(nsub), nchg(nsub);
    int rounds_local = 0, rounds_global = 0;
    // round 0 and the local rounds
    for (const JpegSyncSeq& sq : T.seqs) {
        const JpegSyncSeg& sg = T.segs[sq.seg];
        for (uint32_t t = 0; t < sq.nsub; ++t) {
            const uint32_t li = sq.lsub0 + t;
            X[sq.sub0 + t] = jpeg_sync_walk(f, P.huff, fetch, sg.begin, sg.len, jpeg_sync_end(li, S, sg.len), jpeg_sync_guess(fetch, sg.begin, li, S),
                                            E[sq.sub0 + t], nullptr, (JpegPosBits<JpegFetchBytes>*)nullptr);
            chg[sq.sub0 + t] = 1;
        }
        for (int r = 1; r < Q; ++r) {
            bool any = false;
            for (uint32_t t = 0; t < sq.nsub; ++t) {
                const uint32_t i = sq.sub0 + t;
                nx[i] = X[i]; nchg[i] = 0;
                if (!t || !chg[i - 1]) continue;
                nx[i] = jpeg_sync_walk(f, P.huff, fetch, sg.begin, sg.len, jpeg_sync_end(sq.lsub0 + t, S, sg.len), X[i - 1], E[i], nullptr,
                                       (JpegPosBits<JpegFetchBytes>*)nullptr);
                nchg[i] = !jpeg_sync_same(nx[i], X[i]);
                any = any || nchg[i];
            }
            for (uint32_t t = 0; t < sq.nsub; ++t) { X[sq.sub0 + t] = nx[sq.sub0 + t]; chg[sq.sub0 + t] = nchg[sq.sub0 + t]; }
            if (!any) break;
            if (r > rounds_local) rounds_local = r;
        }
    }
    // global rounds
    std::vector<uint8_t> mark(nseq), nmark(nseq);
    std::vector<JpegSyncState> entry(nseq);
    bool any = false;
    for (uint32_t q = 0; q < nseq; ++q) { mark[q] = T.seqs[q].lsub0 != 0u; any = any || mark[q]; }
    for (uint32_t r = 1; r <= nseq && any; ++r) {
        for (uint32_t q = 0; q < nseq; ++q) if (mark[q]) entry[q] = X[T.seqs[q].sub0 - 1];
        bool wrote = false;
        any = false;
        for (uint32_t q = 0; q < nseq; ++q) {
            nmark[q] = 0;
        }
        for (uint32_t q = 0; q < nseq; ++q) {
            if (!mark[q]) continue;
            const JpegSyncSeq& sq = T.seqs[q];
            const JpegSyncSeg& sg = T.segs[sq.seg];
            JpegSyncState in = entry[q];
            for (uint32_t t = 0; t < sq.nsub; ++t) {
                const uint32_t i = sq.sub0 + t;
                const JpegSyncState x = jpeg_sync_walk(f, P.huff, fetch, sg.begin, sg.len, jpeg_sync_end(sq.lsub0 + t, S, sg.len), in, E[i], nullptr,
                                                       (JpegPosBits<JpegFetchBytes>*)nullptr);
                if (jpeg_sync_same(x, X[i])) break;
                X[i] = x; in = x; wrote = true;
                if (t + 1 == sq.nsub && q + 1 < nseq && T.seqs[q + 1].seg == sq.seg) { nmark[q + 1] = 1; any = true; }
            }
        }
        mark.swap(nmark);
        if (wrote) rounds_global = (int)r;
    }
    // block indices and the write pass
    uint32_t key = 0xFFFFFFFFu;
    for (uint32_t q = 0; q < nseq; ++q) {
        const JpegSyncSeq& sq = T.seqs[q];
        const JpegSyncSeg& sg = T.segs[sq.seg];
        for (uint32_t t = 0; t < sq.nsub; ++t) {
            const uint32_t i = sq.sub0 + t, li = sq.lsub0 + t;
            B[i] = li ? B[i - 1] + E[i - 1] : sg.blk0;
            const uint32_t k = jpeg_sync_write_lane(f, P.huff, fetch, sg, sq, t, li ? X[i - 1] : JpegSyncState{0u, 0u}, B[i]);
            if (k < key) key = k;
            if (states) {
                const JpegSyncState e = li ? X[i - 1] : JpegSyncState{0u, 0u};
                states[i] = mi355_jpeg_sync_state{(int)sq.seg, e.byte, (int)(e.meta & 7u), (int)((e.meta >> 3) & 7u), (int)(e.meta >> 6), B[i]};
            }
        }
    }
    // the DC pass
    for (int c = 0; c < f.ncomp; ++c) {
        uint32_t run = 0;
        const long long ne = jpeg_sync_dc_count(f, c);
        for (long long e = 0; e < ne; ++e) {
            bool first;
            int16_t* dc = coef + jpeg_sync_dc_block(f, c, e, first) * 64;
            run = (first ? 0u : run) + (uint32_t)(int)*dc;
            *dc = (int16_t)(uint16_t)run;
        }
    }
    if (stats) *stats = mi355_jpeg_sync_stats{(int)nsub, (int)nseq, rounds_local, rounds_global};
    return key == 0xFFFFFFFFu ? kJpegDecOk : (int)(key & 7u);
}
}  // namespace mi355
