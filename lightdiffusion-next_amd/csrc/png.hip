// SaveImage, the last stage of every pipeline exit (src/FileManaging/ImageSaver.py:79-220: clip(i * 255, 0, 255).astype(uint8), Image.fromarray,
// img.save(compress_level=4)), on HWC images of the device: the finished PNG file in three launches per call.  include/ldx.h states the format rules;
// lightdiffusion-next_amd/png.py (png_host) is the same thing in numpy, and the bytes are equal.  Plain C++, linked into libldx_png.so (csrc/Makefile
// says why).  Everything is integer work and a pure function of the bytes, so the order of the threads does not show in the file.
//
//   png_filter_kernel   one workgroup per image row: quantise, the five filters' costs, the row of the cheapest into the filtered stream
//   png_deflate_kernel  one workgroup of 1024 per PNG_CHUNK bytes of the stream, the chunk and its deflate bytes both in LDS (50 448 B: three
//                       workgroups share a CU's 160 KiB): matcher, histogram, code lengths, header, bit packing by prefix sum, the chunk's CRC-32 and Adler-32 sums
//   png_pack_kernel     one workgroup per chunk moves it to its prefix-summed offset; one more writes signature, IHDR, the Adler-32, IEND, the length
#include "../../include/ldx.h"
#include "ldx_kernels.h"

namespace ldx {

// bytes of the filtered stream per deflate block (png.py: CHUNK).  Measured at 1024^2 on one MI355X (profiles/png_probe.py): 16 KiB chunks (193 workgroups
// for 256 CUs) encode in 0.22-0.28 ms and 32 KiB chunks (97) in 0.34-0.39 ms; the 16 KiB files are 0.3-0.7 % larger.
constexpr int PNG_CHUNK = 16384;
constexpr int PNG_THREADS = 1024;
constexpr int PNG_PER = PNG_CHUNK / PNG_THREADS;    // positions per thread
constexpr int PNG_SLOT = PNG_CHUNK + 16;            // bytes kept per chunk's deflate output: at most the chunk + 11 (the bound in ldx.h + the zlib header)
constexpr int PNG_MAX_MATCH = 258;
constexpr unsigned PNG_ADLER = 65521u;
constexpr unsigned PNG_CRC_POLY = 0xEDB88320u;
constexpr int PNG_LL = 286, PNG_CL = 19;

// what a chunk's workgroup leaves for the pack kernel
struct PngChunkMeta { unsigned len, crc, a, b; };   // deflate bytes in the slot; CRC-32 of "IDAT" + those bytes; the chunk's Adler sums mod 65521

// ---- CRC-32 (reflected, polynomial 0xEDB88320): registers of byte slices combined by multiplication with x^(8 n) ------------------------------------
// a * b mod P in the reflected representation (bit 31 is x^0): 32 steps, no carry-less multiply
__host__ __device__ constexpr unsigned png_gf2_mul(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PNG_CRC_POLY : b >> 1;
    }
    return p;
}
struct PngPowers { unsigned v[32]; };
constexpr PngPowers png_make_powers() {             // v[k] = x^(8 * 2^k) mod P
    PngPowers t{};
    t.v[0] = 0x00800000u;                           // x^8
    for (int k = 1; k < 32; ++k) t.v[k] = png_gf2_mul(t.v[k - 1], t.v[k - 1]);
    return t;
}
__device__ const PngPowers png_powers = png_make_powers();
// the order in which a dynamic block's header lists the lengths of the code-length code (RFC 1951 3.2.7)
__device__ const unsigned char png_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
// a slice's register moved past the `nbytes` that follow the slice (the other slices account for their content): reg * x^(8 nbytes) mod P
__device__ __forceinline__ unsigned png_crc_shift(unsigned reg, unsigned nbytes) {
    for (int k = 0; nbytes; ++k, nbytes >>= 1)
        if (nbytes & 1u) reg = png_gf2_mul(reg, png_powers.v[k]);
    return reg;
}
__device__ __forceinline__ unsigned png_crc_byte_slow(unsigned reg, unsigned byte) {
    reg ^= byte;
    for (int i = 0; i < 8; ++i) reg = (reg & 1u) ? (reg >> 1) ^ PNG_CRC_POLY : reg >> 1;
    return reg;
}
__device__ __forceinline__ void png_store_be32(uint8_t* p, unsigned v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// ---- stage 1: quantise and filter -----------------------------------------------------------------------------------------------------------------
// the reference's fp32 -> uint8: (uint8) trunc(clamp(255.0f * v, 0, 255)); NaN -> 0 (ldx_hdr_apply's rule)
__device__ __forceinline__ int png_quantize(float v) {
    float c = v * 255.0f;
    c = c >= 0.0f ? c : 0.0f;
    c = c <= 255.0f ? c : 255.0f;
    return (int)c;
}
__device__ __forceinline__ int png_abs(int v) { return v < 0 ? -v : v; }
// the residual of filter `type` (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) of byte x against a = left, b = up, c = upper left
__device__ __forceinline__ int png_residual(int type, int x, int a, int b, int c) {
    int pred = 0;
    if (type == 1) pred = a;
    else if (type == 2) pred = b;
    else if (type == 3) pred = (a + b) >> 1;
    else if (type == 4) {
        const int p = a + b - c, pa = png_abs(p - a), pb = png_abs(p - b), pc = png_abs(p - c);
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (x - pred) & 255;
}
// grid (H, B), 256 threads; LDS: the five costs (20 B)
template <bool F32>
__global__ __launch_bounds__(256) void png_filter_kernel(const float* __restrict__ in_f, const uint8_t* __restrict__ in_u, long in_pitch, int H, int W,
                                                         uint8_t* __restrict__ stream, uint8_t* __restrict__ types) {
    __shared__ unsigned cost[5];
    const int y = blockIdx.x, b = blockIdx.y, rowlen = 3 * W;
    const float* rf = F32 ? in_f + ((long)b * H + y) * rowlen : nullptr;
    const uint8_t* ru = F32 ? nullptr : in_u + ((long)b * H + y) * in_pitch;
    const long up = F32 ? (long)rowlen : in_pitch;                      // elements back to the row above
    auto at = [&](int x, bool above) -> int {
        if (above && y == 0) return 0;
        if (F32) return png_quantize(rf[x - (above ? up : 0)]);
        return (int)ru[x - (above ? up : 0)];
    };
    if (threadIdx.x < 5) cost[threadIdx.x] = 0;
    __syncthreads();
    unsigned sum[5] = {0, 0, 0, 0, 0};
    for (int x = threadIdx.x; x < rowlen; x += 256) {
        const int v = at(x, false), a = x >= 3 ? at(x - 3, false) : 0, u = at(x, true), c = x >= 3 ? at(x - 3, true) : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int r = png_residual(t, v, a, u, c);
            sum[t] += (unsigned)(r < 128 ? r : 256 - r);
        }
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) atomicAdd(&cost[t], sum[t]);
    __syncthreads();
    int type = 0;
#pragma unroll
    for (int t = 1; t < 5; ++t) if (cost[t] < cost[type]) type = t;    // ties to the lowest type
    uint8_t* dst = stream + ((long)b * H + y) * (1 + rowlen);
    if (threadIdx.x == 0) { dst[0] = (uint8_t)type; if (types) types[(long)b * H + y] = (uint8_t)type; }
    for (int x = threadIdx.x; x < rowlen; x += 256) {
        const int v = at(x, false), a = x >= 3 ? at(x - 3, false) : 0, u = at(x, true), c = x >= 3 ? at(x - 3, true) : 0;
        dst[1 + x] = (uint8_t)png_residual(type, v, a, u, c);
    }
}

// ---- stage 2: deflate -------------------------------------------------------------------------------------------------------------------------------
// inclusive scan over the workgroup's 1024 values in LDS (buf: 2 x 1024 words), from thread 0 up or, reversed, from thread 1023 down; every thread calls it
template <class Op>
__device__ __forceinline__ unsigned png_block_scan(unsigned v, unsigned* buf, bool reversed, Op op) {
    const int t = reversed ? PNG_THREADS - 1 - (int)threadIdx.x : (int)threadIdx.x;
    unsigned* a = buf;
    unsigned* b = buf + PNG_THREADS;
    __syncthreads();                                // the buffer may still be read from the scan before
    a[t] = v;
    __syncthreads();
    for (int o = 1; o < PNG_THREADS; o <<= 1) {
        unsigned x = a[t];
        if (t >= o) x = op(a[t - o], x);
        b[t] = x;
        __syncthreads();
        unsigned* s = a; a = b; b = s;
    }
    return a[t];
}

// The matcher, per position p of the span [p0, p1) of a chunk s[0..n): f(p, literal byte, 0) or f(p, -1, match length).  A position breaks when it is
// the chunk's first or differs from the byte before.  Otherwise it lies in a run: a = the last break before it, R = nb - a - 1 positions up to the
// next break nb (or n), k = p - a - 1.  R < 4: literal.  Else the run is cut into pieces of 258: a piece < 3 is literals, any other one match at its
// first position.  prevb = the last break before p0 (unused when p0 is itself a break), nextb = the first break at or after p1, or n.
template <class F>
__device__ __forceinline__ void png_walk(const uint8_t* s, int p0, int p1, int prevb, int nextb, F f) {
    auto find = [&](int q) {
        while (q < p1 && q != 0 && s[q] == s[q - 1]) ++q;
        return q < p1 ? q : nextb;
    };
    int a = prevb, nb = find(p0);
    for (int p = p0; p < p1; ++p) {
        if (p == nb) { a = p; nb = find(p + 1); f(p, (int)s[p], 0); continue; }
        const int k = p - a - 1, R = nb - a - 1;
        const int base = (k / PNG_MAX_MATCH) * PNG_MAX_MATCH;
        const int piece = R - base < PNG_MAX_MATCH ? R - base : PNG_MAX_MATCH;
        if (R >= 4 && piece >= 3) { if (k == base) f(p, -1, piece); }
        else f(p, (int)s[p], 0);
    }
}
// RFC 1951's length codes by arithmetic: length 3..258 -> code index 0..28, number of extra bits, their value
__device__ __forceinline__ void png_length_code(int len, int& idx, int& ebits, int& eval) {
    const int v = len - 3;
    if (len == PNG_MAX_MATCH) { idx = 28; ebits = 0; eval = 0; return; }
    if (v < 8) { idx = v; ebits = 0; eval = 0; return; }
    ebits = (31 - __clz(v)) - 2;
    idx = 4 * ebits + 4 + ((v >> ebits) & 3);
    eval = v & ((1 << ebits) - 1);
}

// LDS of the code construction (png.py: huffman_lengths, canonical_codes)
struct PngHuff {
    unsigned w[PNG_LL], iw[PNG_LL];                 // weights of the sorted leaves and of the internal nodes, in order of creation
    unsigned short order[PNG_LL], lp[PNG_LL], ip[PNG_LL], dep[PNG_LL];      // sorted leaf -> symbol; parents of leaves and internal nodes; depths
    unsigned num[16], cum[16], next[16];
    unsigned used;
};
// Code lengths <= limit of the nsym <= 286 symbols with a non-zero count, every thread of the workgroup calling.  The used symbols sorted by
// (count, symbol); Huffman's algorithm on two queues, a leaf before an internal node of equal weight; depths above the limit set to it and the
// number of codes per length repaired (while the Kraft sum is above 1: one code of the limit leaves, the deepest shorter code moves one down and
// takes the leaver along); the lengths go to the symbols in sorted order, the rarest the longest.  Then canonical codes, bit-reversed.
__device__ void png_huffman(const unsigned* cnt, int nsym, int limit, unsigned short* len, unsigned short* code, PngHuff& h) {
    const int t = threadIdx.x;
    if (t == 0) h.used = 0;
    if (t < 16) h.num[t] = 0;
    __syncthreads();
    if (t < nsym) {
        len[t] = 0; code[t] = 0;
        const unsigned c = cnt[t];
        if (c) {
            int r = 0;
            for (int j = 0; j < nsym; ++j) { const unsigned d = cnt[j]; r += (d != 0 && (d < c || (d == c && j < t))) ? 1 : 0; }
            h.order[r] = (unsigned short)t; h.w[r] = c;
            atomicAdd(&h.used, 1u);
        }
    }
    __syncthreads();
    const int u = (int)h.used;
    if (u == 0) return;
    if (u == 1) {
        if (t == 0) len[h.order[0]] = 1;            // its code is 0
        __syncthreads();
        return;
    }
    if (t == 0) {
        int li = 0, ii = 0;
        for (int j = 0; j < u - 1; ++j) {
            unsigned s = 0;
            for (int r = 0; r < 2; ++r) {
                if (li < u && (ii >= j || h.w[li] <= h.iw[ii])) { s += h.w[li]; h.lp[li] = (unsigned short)j; ++li; }
                else { s += h.iw[ii]; h.ip[ii] = (unsigned short)j; ++ii; }
            }
            h.iw[j] = s;
        }
        h.dep[u - 2] = 0;
        for (int j = u - 3; j >= 0; --j) h.dep[j] = (unsigned short)(h.dep[h.ip[j]] + 1);
    }
    __syncthreads();
    if (t < u) { const int d = h.dep[h.lp[t]] + 1; atomicAdd(&h.num[d < limit ? d : limit], 1u); }
    __syncthreads();
    if (t == 0) {
        unsigned total = 0;
        for (int i = 1; i <= limit; ++i) total += h.num[i] << (limit - i);
        while (total > (1u << limit)) {
            h.num[limit] -= 1;
            for (int i = limit - 1; i > 0; --i)
                if (h.num[i]) { h.num[i] -= 1; h.num[i + 1] += 2; break; }
            total -= 1;
        }
        unsigned c = 0, nx = 0;
        h.cum[0] = 0; h.next[0] = 0;
        for (int i = 1; i <= limit; ++i) {
            nx = (nx + h.num[i - 1]) << 1;          // num[0] is 0
            h.next[i] = nx;
            c += h.num[i]; h.cum[i] = c;
        }
    }
    __syncthreads();
    if (t < u) {
        const unsigned dd = (unsigned)(u - 1 - t);
        int L = 1;
        while (h.cum[L] <= dd) ++L;
        len[h.order[t]] = (unsigned short)L;
    }
    __syncthreads();
    if (t < nsym) {
        const int L = len[t];
        if (L) {
            unsigned c = h.next[L];
            for (int j = 0; j < t; ++j) c += len[j] == L ? 1u : 0u;
            code[t] = (unsigned short)(__brev(c) >> (32 - L));
        }
    }
    __syncthreads();
}

// `nb` bits of val at bit `pos` of the zeroed word array, least significant first; fields of different threads meet in a word, so the words are or-ed
__device__ __forceinline__ void png_put(unsigned* out, unsigned pos, unsigned val, int nb) {
    if (nb == 0) return;
    const unsigned long long v = (unsigned long long)val << (pos & 31u);
    atomicOr(&out[pos >> 5], (unsigned)v);
    const unsigned hi = (unsigned)(v >> 32);
    if (hi) atomicOr(&out[(pos >> 5) + 1], hi);
}

// grid (nchunks, B), 1024 threads.  src: B streams of N bytes, `src_stride` apart; chunk c of stream b goes to slots[(b * nchunks + c) * PNG_SLOT] and
// meta[b * nchunks + c].  with_crc: the CRC-32 of "IDAT" + the chunk's deflate bytes is wanted.
// LDS 50 448 B: the chunk 16 384, the deflate bytes 16 400, the scan buffer 8 192, code construction and tables 9 472.
__global__ __launch_bounds__(PNG_THREADS) void png_deflate_kernel(const uint8_t* __restrict__ src, long src_stride, long N, int nchunks,
                                                                  uint8_t* __restrict__ slots, PngChunkMeta* __restrict__ meta, int with_crc) {
    __shared__ unsigned s_in_w[PNG_CHUNK / 4];
    __shared__ unsigned s_out[PNG_SLOT / 4];
    __shared__ unsigned s_scan[2 * PNG_THREADS];
    __shared__ PngHuff s_h;
    __shared__ unsigned s_cnt[PNG_LL + 2];
    __shared__ unsigned short s_len[PNG_LL + 2], s_code[PNG_LL + 2];    // literal / length code; the two distance lengths follow at [nlit], [nlit + 1]
    __shared__ unsigned s_clcnt[PNG_CL];
    __shared__ unsigned short s_cllen[PNG_CL], s_clcode[PNG_CL];
    __shared__ unsigned s_rle[PNG_LL + 2];                              // symbol | extra value << 8 | extra bits << 16
    __shared__ unsigned s_crc[256];
    __shared__ unsigned s_var[8];                                       // 0 tokens of the header, 1 nlit, 2 ncl, 3 header bits, 4 crc, 5 adler a, 6 adler b
    uint8_t* const s = (uint8_t*)s_in_w;
    uint8_t* const ob = (uint8_t*)s_out;
    const int t = threadIdx.x, c = blockIdx.x, b = blockIdx.y;
    const long start = (long)c * PNG_CHUNK;
    const int n = (int)(N - start < PNG_CHUNK ? N - start : PNG_CHUNK);
    const bool last = c == nchunks - 1;
    const uint8_t* g = src + (long)b * src_stride + start;

    for (int i = t; i < n; i += PNG_THREADS) s[i] = g[i];
    for (int i = t; i < PNG_LL + 2; i += PNG_THREADS) s_cnt[i] = 0;
    if (t < PNG_CL) s_clcnt[t] = 0;
    if (t < 8) s_var[t] = 0;
    if (t < 256) {
        unsigned r = (unsigned)t;
        for (int i = 0; i < 8; ++i) r = (r & 1u) ? (r >> 1) ^ PNG_CRC_POLY : r >> 1;
        s_crc[t] = r;
    }
    __syncthreads();

    // the breaks around this thread's span
    const int p0 = t * PNG_PER < n ? t * PNG_PER : n, p1 = (t + 1) * PNG_PER < n ? (t + 1) * PNG_PER : n;
    int firstb = n, lastb = -1;
    for (int p = p0; p < p1; ++p)
        if (p == 0 || s[p] != s[p - 1]) { if (firstb == n) firstb = p; lastb = p; }
    // the last break in the spans up to t: a running maximum (+ 1, so that 0 is "none"); the first break in the spans from t on: a running minimum from the
    // right; each thread then takes its neighbours' values
    const unsigned upto = png_block_scan((unsigned)(lastb + 1), s_scan, false, [](unsigned x, unsigned y) { return x > y ? x : y; });
    const unsigned from = png_block_scan((unsigned)firstb, s_scan, true, [](unsigned x, unsigned y) { return x < y ? x : y; });
    __syncthreads();
    s_scan[t] = upto; s_scan[PNG_THREADS + t] = from;
    __syncthreads();
    const int prevb = t == 0 ? -1 : (int)s_scan[t - 1] - 1;
    const int nextb = t + 1 < PNG_THREADS ? (int)s_scan[PNG_THREADS + t + 1] : n;

    // histogram of the literal / length alphabet
    png_walk(s, p0, p1, prevb, nextb, [&](int, int lit, int len) {
        int sym = lit;
        if (len) { int idx, eb, ev; png_length_code(len, idx, eb, ev); sym = 257 + idx; }
        atomicAdd(&s_cnt[sym], 1u);
    });
    if (t == 0) atomicAdd(&s_cnt[256], 1u);
    __syncthreads();
    png_huffman(s_cnt, PNG_LL, 15, s_len, s_code, s_h);

    // the code lengths as symbols of the code-length alphabet (png.py: _code_length_tokens), greedy from the left
    if (t == 0) {
        int nlit = PNG_LL;
        while (nlit > 257 && s_len[nlit - 1] == 0) --nlit;
        s_len[nlit] = 1; s_len[nlit + 1] = 1;                           // two distance codes of one bit: distance 1 is the bit 0
        const int total = nlit + 2;
        int ntok = 0;
        for (int i = 0; i < total;) {
            const int v = s_len[i];
            int r = 1;
            while (i + r < total && s_len[i + r] == v && r < 138) ++r;
            unsigned tok;
            if (v == 0 && r >= 11) { tok = 18u | (unsigned)(r - 11) << 8 | 7u << 16; i += r; }
            else if (v == 0 && r >= 3) { tok = 17u | (unsigned)(r - 3) << 8 | 3u << 16; i += r; }
            else if (v != 0 && i > 0 && s_len[i - 1] == v && r >= 3) { r = r < 6 ? r : 6; tok = 16u | (unsigned)(r - 3) << 8 | 2u << 16; i += r; }
            else { tok = (unsigned)v; i += 1; }
            s_rle[ntok++] = tok;
            s_clcnt[tok & 255u] += 1;
        }
        s_var[0] = (unsigned)ntok; s_var[1] = (unsigned)nlit;
    }
    __syncthreads();
    png_huffman(s_clcnt, PNG_CL, 7, s_cllen, s_clcode, s_h);
    if (t == 0) {
        int ncl = PNG_CL;
        while (ncl > 4 && s_cllen[png_cl_order[ncl - 1]] == 0) --ncl;
        unsigned bits = 3 + 5 + 5 + 4 + 3 * (unsigned)ncl;
        for (unsigned i = 0; i < s_var[0]; ++i) bits += s_cllen[s_rle[i] & 255u] + (s_rle[i] >> 16);
        s_var[2] = (unsigned)ncl; s_var[3] = bits;
    }

    // bits of this thread's tokens, their prefix sum
    unsigned mybits = 0;
    png_walk(s, p0, p1, prevb, nextb, [&](int, int lit, int len) {
        if (len) { int idx, eb, ev; png_length_code(len, idx, eb, ev); mybits += s_len[257 + idx] + eb + 1; }
        else mybits += s_len[lit];
    });
    const unsigned incl_bits = png_block_scan(mybits, s_scan, false, [](unsigned x, unsigned y) { return x + y; });
    __syncthreads();
    if (t == PNG_THREADS - 1) s_var[7] = incl_bits;
    __syncthreads();
    const unsigned all_tok_bits = s_var[7];
    const unsigned head = c == 0 ? 2u : 0u;                             // the zlib header 78 01 opens the first chunk
    const unsigned dyn_bits = s_var[3] + all_tok_bits + s_len[256];
    const unsigned dyn_bytes = (dyn_bits + 7) / 8;
    unsigned m;                                                         // bytes this chunk leaves
    for (int i = t; i < PNG_SLOT / 4; i += PNG_THREADS) s_out[i] = 0;
    __syncthreads();
    if (t == 0 && head) { ob[0] = 0x78; ob[1] = 0x01; }
    __syncthreads();
    if (dyn_bytes < (unsigned)n + 5) {
        const unsigned bit0 = head * 8;
        if (t == 0) {
            unsigned pos = bit0;
            png_put(s_out, pos, last ? 1u : 0u, 1); pos += 1;
            png_put(s_out, pos, 2u, 2); pos += 2;
            png_put(s_out, pos, s_var[1] - 257, 5); pos += 5;
            png_put(s_out, pos, 1u, 5); pos += 5;
            png_put(s_out, pos, s_var[2] - 4, 4); pos += 4;
            for (unsigned i = 0; i < s_var[2]; ++i) { png_put(s_out, pos, s_cllen[png_cl_order[i]], 3); pos += 3; }
            for (unsigned i = 0; i < s_var[0]; ++i) {
                const unsigned tok = s_rle[i], sym = tok & 255u, L = s_cllen[sym], eb = tok >> 16;
                png_put(s_out, pos, s_clcode[sym] | ((tok >> 8) & 255u) << L, (int)(L + eb)); pos += L + eb;
            }
            png_put(s_out, bit0 + s_var[3] + all_tok_bits, s_code[256], s_len[256]);
        }
        unsigned pos = bit0 + s_var[3] + incl_bits - mybits;
        png_walk(s, p0, p1, prevb, nextb, [&](int, int lit, int len) {
            if (len) {
                int idx, eb, ev; png_length_code(len, idx, eb, ev);
                const unsigned L = s_len[257 + idx];
                png_put(s_out, pos, s_code[257 + idx] | (unsigned)ev << L, (int)(L + eb + 1));          // the distance bit 0 on top
                pos += L + eb + 1;
            } else { png_put(s_out, pos, s_code[lit], s_len[lit]); pos += s_len[lit]; }
        });
        const unsigned end_bits = bit0 + dyn_bits;
        if (last) m = (end_bits + 7) / 8;
        else {                                                          // an empty stored block: 000, to the byte boundary, 00 00 FF FF
            const unsigned q = (end_bits + 3 + 7) / 8;
            m = q + 4;
            __syncthreads();
            if (t == 0) { ob[q + 2] = 0xFF; ob[q + 3] = 0xFF; }
        }
    } else {                                                            // stored: BFINAL, LEN, ~LEN, the bytes
        if (t == 0) {
            ob[head] = last ? 1 : 0;
            ob[head + 1] = (uint8_t)n; ob[head + 2] = (uint8_t)(n >> 8); ob[head + 3] = (uint8_t)~n; ob[head + 4] = (uint8_t)(~n >> 8);
        }
        for (int p = p0; p < p1; ++p) ob[head + 5 + p] = s[p];
        m = head + 5 + (unsigned)n;
    }
    __syncthreads();

    // CRC-32 of "IDAT" + the m bytes: every thread the register of its slice, moved to the end by x^(8 * bytes after it); Adler sums of the chunk
    if (with_crc) {
        const unsigned sl = (m + PNG_THREADS - 1) / PNG_THREADS;
        const unsigned q0 = (unsigned)t * sl < m ? (unsigned)t * sl : m, q1 = (unsigned)(t + 1) * sl < m ? (unsigned)(t + 1) * sl : m;
        unsigned reg = 0;
        if (t == 0) {
            reg = 0xFFFFFFFFu;
            reg = s_crc[(reg ^ 0x49u) & 255u] ^ (reg >> 8); reg = s_crc[(reg ^ 0x44u) & 255u] ^ (reg >> 8);          // "IDAT"
            reg = s_crc[(reg ^ 0x41u) & 255u] ^ (reg >> 8); reg = s_crc[(reg ^ 0x54u) & 255u] ^ (reg >> 8);
        }
        for (unsigned q = q0; q < q1; ++q) reg = s_crc[(reg ^ ob[q]) & 255u] ^ (reg >> 8);
        if (reg) atomicXor(&s_var[4], png_crc_shift(reg, m - q1));
    }
    unsigned sa = 0, sb = 0;
    for (int p = p0; p < p1; ++p) { sa += s[p]; sb += (unsigned)(n - p) * s[p]; }
    atomicAdd(&s_var[5], sa);
    atomicAdd(&s_var[6], sb % PNG_ADLER);
    __syncthreads();
    const long slot = (long)b * nchunks + c;
    unsigned* dst = (unsigned*)(slots + slot * PNG_SLOT);
    for (unsigned i = t; i < (m + 3) / 4; i += PNG_THREADS) dst[i] = s_out[i];
    if (t == 0) {
        PngChunkMeta r;
        r.len = m; r.crc = s_var[4] ^ 0xFFFFFFFFu; r.a = s_var[5] % PNG_ADLER; r.b = s_var[6] % PNG_ADLER;
        meta[slot] = r;
    }
}

// ---- stage 3: container -------------------------------------------------------------------------------------------------------------------------------
// grid (nchunks + 1, B), 256 threads.  framed: a PNG (H, W for IHDR); otherwise the bare zlib stream.  Block c < nchunks moves chunk c to its offset;
// block nchunks writes what stands around the chunks and the length.  LDS: three 64-bit sums (24 B).
__global__ __launch_bounds__(256) void png_pack_kernel(const uint8_t* __restrict__ slots, const PngChunkMeta* __restrict__ meta, int nchunks, long N,
                                                       int H, int W, int framed, uint8_t* __restrict__ out, long out_stride, unsigned* __restrict__ out_len) {
    __shared__ unsigned long long acc[3];                               // bytes before this chunk; the Adler sums
    const int t = threadIdx.x, c = blockIdx.x, b = blockIdx.y;
    const PngChunkMeta* mt = meta + (long)b * nchunks;
    uint8_t* o = out + (long)b * out_stride;
    const unsigned frame = framed ? 12u : 0u;
    unsigned long long before = 0;
    for (int j = t; j < c && j < nchunks; j += 256) before += mt[j].len + frame;
    unsigned long long pa = 0, pb = 0;
    if (c == nchunks)               // Adler-32 of the N bytes from the chunks' sums: A = 1 + sum a_j, B = N + sum (b_j + a_j * bytes after chunk j), mod 65521
        for (int j = t; j < nchunks; j += 256) {
            const long end = (long)(j + 1) * PNG_CHUNK < N ? (long)(j + 1) * PNG_CHUNK : N;
            pa += mt[j].a;
            pb += mt[j].b + (unsigned long long)mt[j].a * (unsigned long long)((N - end) % PNG_ADLER) % PNG_ADLER;
        }
    if (t < 3) acc[t] = 0;
    __syncthreads();
    atomicAdd(&acc[0], before); atomicAdd(&acc[1], pa); atomicAdd(&acc[2], pb);
    __syncthreads();
    const unsigned long long off = (framed ? 33u : 0u) + acc[0], sa = acc[1], sb = acc[2];
    if (c < nchunks) {
        const unsigned m = mt[c].len;
        const uint8_t* src = slots + ((long)b * nchunks + c) * PNG_SLOT;
        uint8_t* d = o + off;
        if (framed) {
            if (t == 0) { png_store_be32(d, m); d[4] = 0x49; d[5] = 0x44; d[6] = 0x41; d[7] = 0x54; png_store_be32(d + 8 + m, mt[c].crc); }
            d += 8;
        }
        for (unsigned i = t; i < m; i += 256) d[i] = src[i];
        return;
    }
    if (t != 0) return;
    const unsigned adler = (unsigned)((sb + (unsigned long long)(N % PNG_ADLER)) % PNG_ADLER) << 16 | (unsigned)((sa + 1) % PNG_ADLER);
    uint8_t* d = o + off;
    if (!framed) {
        png_store_be32(d, adler);
        out_len[b] = (unsigned)(off + 4);
        return;
    }
    o[0] = 0x89; o[1] = 0x50; o[2] = 0x4E; o[3] = 0x47; o[4] = 0x0D; o[5] = 0x0A; o[6] = 0x1A; o[7] = 0x0A;
    png_store_be32(o + 8, 13);
    o[12] = 0x49; o[13] = 0x48; o[14] = 0x44; o[15] = 0x52;                                            // IHDR: W, H, 8 bits, colour type 2, 0, 0, 0
    png_store_be32(o + 16, (unsigned)W); png_store_be32(o + 20, (unsigned)H);
    o[24] = 8; o[25] = 2; o[26] = 0; o[27] = 0; o[28] = 0;
    unsigned reg = 0xFFFFFFFFu;
    for (int i = 12; i < 29; ++i) reg = png_crc_byte_slow(reg, o[i]);
    png_store_be32(o + 29, reg ^ 0xFFFFFFFFu);
    png_store_be32(d, 4);                                                                               // the Adler-32 in an IDAT of its own
    d[4] = 0x49; d[5] = 0x44; d[6] = 0x41; d[7] = 0x54;
    png_store_be32(d + 8, adler);
    reg = 0xFFFFFFFFu;
    for (int i = 4; i < 12; ++i) reg = png_crc_byte_slow(reg, d[i]);
    png_store_be32(d + 12, reg ^ 0xFFFFFFFFu);
    png_store_be32(d + 16, 0);                                                                          // IEND
    d[20] = 0x49; d[21] = 0x45; d[22] = 0x4E; d[23] = 0x44;
    png_store_be32(d + 24, 0xAE426082u);
    out_len[b] = (unsigned)(off + 28);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------------
static long png_round256(long v) { return (v + 255) / 256 * 256; }
long png_stream_bytes(int H, int W) { return (long)H * (1 + 3L * W); }
long png_chunks(long n) { return (n + PNG_CHUNK - 1) / PNG_CHUNK; }
// workspace of the deflate + pack stages for B streams of n bytes: the chunks' meta records, then their slots
static long png_deflate_workspace(int B, long n) { return png_round256((long)B * png_chunks(n) * (long)sizeof(PngChunkMeta)) + (long)B * png_chunks(n) * PNG_SLOT; }
long png_workspace_bytes(int B, int H, int W) { return png_round256((long)B * png_stream_bytes(H, W)) + png_deflate_workspace(B, png_stream_bytes(H, W)); }
long png_bound_bytes(int H, int W) { const long n = png_stream_bytes(H, W); return 63 + n + 21 * png_chunks(n); }
long zlib_workspace_bytes(long n) { return png_deflate_workspace(1, n); }
long zlib_bound_bytes(long n) { return 6 + n + 9 * png_chunks(n); }

void launch_png_filter(const float* in_f32, const uint8_t* in_u8, long in_pitch, int B, int H, int W, uint8_t* stream, uint8_t* types, hipStream_t s) {
    if (in_f32) hipLaunchKernelGGL(png_filter_kernel<true>, dim3(H, B), dim3(256), 0, s, in_f32, (const uint8_t*)nullptr, 0L, H, W, stream, types);
    else hipLaunchKernelGGL(png_filter_kernel<false>, dim3(H, B), dim3(256), 0, s, (const float*)nullptr, in_u8, in_pitch, H, W, stream, types);
}
static void launch_deflate_pack(const uint8_t* src, int B, long n, int H, int W, int framed, void* workspace, uint8_t* out, long out_stride,
                                uint32_t* out_len, hipStream_t s) {
    const int nchunks = (int)png_chunks(n);
    PngChunkMeta* meta = (PngChunkMeta*)workspace;
    uint8_t* slots = (uint8_t*)workspace + png_round256((long)B * nchunks * (long)sizeof(PngChunkMeta));
    hipLaunchKernelGGL(png_deflate_kernel, dim3(nchunks, B), dim3(PNG_THREADS), 0, s, src, n, n, nchunks, slots, meta, framed);
    hipLaunchKernelGGL(png_pack_kernel, dim3(nchunks + 1, B), dim3(256), 0, s, (const uint8_t*)slots, (const PngChunkMeta*)meta, nchunks, n, H, W, framed,
                       out, out_stride, out_len);
}
void launch_png_encode(const PngArgs& a, hipStream_t s) {
    const long n = png_stream_bytes(a.H, a.W);
    uint8_t* stream = (uint8_t*)a.workspace;
    launch_png_filter(a.in_f32, a.in_u8, a.in_pitch, a.B, a.H, a.W, stream, nullptr, s);
    launch_deflate_pack(stream, a.B, n, a.H, a.W, 1, stream + png_round256((long)a.B * n), a.out, a.out_stride, a.out_len, s);
}
void launch_zlib_deflate(const uint8_t* bytes, long n, void* workspace, uint8_t* out, uint32_t* out_len, hipStream_t s) {
    launch_deflate_pack(bytes, 1, n, 0, 0, 0, workspace, out, 0, out_len, s);
}

}  // namespace ldx
