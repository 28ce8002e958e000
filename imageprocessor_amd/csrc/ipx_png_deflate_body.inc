// ipx_png_deflate_body.inc -- the deflate of one segment by one workgroup of kDefThreads lanes: the statements of a kernel's body, not a
// function.  It is included textually inside png_deflate_kernel (ipx_png.hip) and png_mixed_deflate_kernel (ipx_png_mixed.hip) so that
// both run the same statements and the uniform kernel compiles to the instructions it had when the statements stood in it (as a
// __device__ function the compiler laid the same code out 18 % longer).  In scope where it is included:
//   table (uint32_t[kHashSize], LDS), S (DefShared, LDS), t (threadIdx.x), data / M (the frame's filtered stream and match scratch),
//   o (where the segment's IDAT chunk goes), stride, N (the frame's filtered bytes), s0, s1, L, first, last (the segment),
//   lens, adler (the kernel's outputs, indexed by blockIdx.x).
    // ---- 1. candidates: the fixed distances, then the hashed one from a table filled tile by tile
    for (int i = t; i < kHashSize; i += kDefThreads) table[i] = 0;
    __syncthreads();
    for (uint32_t j = (s0 > (uint32_t)kPngWindow ? s0 - kPngWindow : 0) + t; j < s0; j += kDefThreads)
        if (j + 4 <= N) atomicMax(&table[png_hash(data + j)], j + 1);
    __syncthreads();
    int fixed[6], nfixed = 0;
    for (int d = 1; d <= 4; d++) fixed[nfixed++] = d;
    if (stride > 4 && stride <= kPngWindow) fixed[nfixed++] = stride;
    if (2 * stride <= kPngWindow) fixed[nfixed++] = 2 * stride;
    for (uint32_t t0 = s0; t0 < s1; t0 += kPngTile) {
        const uint32_t i = t0 + t;
        if (i < s1) {
            const int cap = (int)min((uint32_t)kPngMaxMatch, s1 - i);
            int best = 0, bd = 0;
            for (int k = 0; k < nfixed && best < cap; k++) {
                const int d = fixed[k];
                if ((uint32_t)d > i) break;
                const int l = match_len(data + i, data + i - d, cap);
                if (l > best) { best = l; bd = d; }
            }
            if (i + 4 <= N) {
                const uint32_t c = table[png_hash(data + i)];
                if (c && i - (c - 1) <= (uint32_t)kPngWindow) {
                    const int d = (int)(i - (c - 1));
                    if (best < cap || d < bd) {
                        const int l = match_len(data + i, data + i - d, cap);
                        if (l > best || (l == best && d < bd)) { best = l; bd = d; }
                    }
                }
            }
            M[i] = best >= kPngMinMatch ? (uint32_t)best << 16 | (uint32_t)(bd - 1) : data[i];
        }
        __syncthreads();
        if (i < s1 && i + 4 <= N) atomicMax(&table[png_hash(data + i)], i + 1);
        __syncthreads();
    }

    // ---- 2. the greedy parse: lane 0 walks windows staged in LDS; tokens go in place to M[s0 + k] (k <= position: never ahead of
    // what is still to be read)
    if (t == 0) { S.ntok = 0; S.p = (int)s0; }
    __syncthreads();
    for (;;) {
        const uint32_t base = (uint32_t)S.p;
        if (base >= s1) break;
        const uint32_t wl = min((uint32_t)kWalkWin, s1 - base);
        for (uint32_t k = t; k < wl; k += kDefThreads) table[k] = M[base + k];
        __syncthreads();
        if (t == 0) {
            uint32_t p = base, nt = (uint32_t)S.ntok;
            while (p < base + wl) {
                const uint32_t m = table[p - base];
                M[s0 + nt++] = m;
                p += m >> 16 ? m >> 16 : 1;
            }
            S.ntok = (int)nt;
            S.p = (int)p;
        }
        __syncthreads();
    }
    const int ntok = S.ntok;

    // ---- 3. histograms and tables
    for (int s = t; s < 286; s += kDefThreads) S.lfreq[s] = 0;
    if (t < 30) S.dfreq[t] = 0;
    if (t < 19) S.cfreq[t] = 0;
    __syncthreads();
    for (int k = t; k < ntok; k += kDefThreads) {
        const uint32_t m = M[s0 + k];
        if (m >> 16) {
            atomicAdd(&S.lfreq[257 + c_png.len_sym[m >> 16]], 1u);
            atomicAdd(&S.dfreq[dist_sym((int)(m & 0xFFFF) + 1)], 1u);
        } else {
            atomicAdd(&S.lfreq[m], 1u);
        }
    }
    __syncthreads();
    if (t == 0) S.lfreq[256] += 1;
    huff_build(S.lfreq, 286, 15, S.llen, S.work);
    huff_build(S.dfreq, 30, 15, S.dlen, S.work);
    if (t == 0) {
        int hlit = 286, hdist = 30;
        while (S.llen[hlit - 1] == 0) hlit--;
        while (hdist > 1 && S.dlen[hdist - 1] == 0) hdist--;
        hlit = max(hlit, 257);
        S.hlit = hlit;
        S.hdist = hdist;
        // run-length code of the hlit + hdist lengths (the model's rle_code_lengths)
        const int n = hlit + hdist;
        int ncl = 0, i = 0;
        auto lenat = [&](int k) { return k < hlit ? S.llen[k] : S.dlen[k - hlit]; };
        auto add = [&](int sym, int x) { S.cl_sym[ncl++] = (uint16_t)(sym | x << 5); S.cfreq[sym]++; };
        while (i < n) {
            const int v = lenat(i);
            int r = 1;
            while (i + r < n && lenat(i + r) == v) r++;
            i += r;
            if (v == 0) {
                while (r >= 11) { const int k = min(r, 138); add(18, k - 11); r -= k; }
                if (r >= 3) { add(17, r - 3); r = 0; }
                for (; r > 0; r--) add(0, 0);
            } else {
                add(v, 0);
                r--;
                while (r >= 3) { const int k = min(r, 6); add(16, k - 3); r -= k; }
                for (; r > 0; r--) add(v, 0);
            }
        }
        S.ncl = ncl;
    }
    huff_build(S.cfreq, 19, 7, S.clen, S.work);
    if (t == 0) {
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 19;
        while (hclen > 4 && S.clen[order[hclen - 1]] == 0) hclen--;
        S.hclen = hclen;
        huff_codes(S.llen, 286, S.lcode);
        huff_codes(S.dlen, 30, S.dcode);
        huff_codes(S.clen, 19, S.ccode);
        unsigned long long hb = (first ? 16 : 0) + 3 + 14 + 3 * hclen;
        for (int k = 0; k < S.ncl; k++) {
            const int sym = S.cl_sym[k] & 31;
            hb += S.clen[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        S.hbits = hb;
    }
    __syncthreads();
    unsigned long long mine = 0;
    for (int k = t; k < ntok; k += kDefThreads) {
        int n;
        (void)token_bits(M[s0 + k], S, &n);
        mine += n;
    }
    const unsigned long long tokbits = block_sum(mine, S.wsum);
    const unsigned long long dynbits = S.hbits + tokbits + S.llen[256] + 3;
    const size_t dyn_bytes = (size_t)((dynbits + 7) / 8) + 4, st_bytes = png_stored_bytes(L, first);
    const bool stored = st_bytes < dyn_bytes;
    const size_t dlen = stored ? st_bytes : dyn_bytes;
    uint8_t *d8 = o + 8;
    uint32_t *dw = (uint32_t *)d8;

    // ---- 4. the bits
    if (stored) {
        const int z = first ? 2 : 0;
        if (t == 0 && first) { d8[0] = 0x78; d8[1] = 0x9C; }
        const uint32_t nblk = (L + 65534) / 65535;
        for (uint32_t b = t; b <= nblk; b += kDefThreads) {
            const uint32_t q0 = min(b * 65535u, L), bl = b == nblk ? 0 : min(65535u, L - q0);
            uint8_t *hp = d8 + z + 5 * b + q0;
            hp[0] = b == nblk && last ? 1 : 0;
            hp[1] = (uint8_t)bl;
            hp[2] = (uint8_t)(bl >> 8);
            hp[3] = (uint8_t)~bl;
            hp[4] = (uint8_t)(~bl >> 8);
        }
        for (uint32_t q = t; q < L; q += kDefThreads) d8[z + 5 * (q / 65535 + 1) + q] = data[s0 + q];
    } else {
        if (t == 0) {
            unsigned long long pos = 0;
            if (first) { put_bits(dw, pos, 0x9C78, 16); pos = 16; }
            put_bits(dw, pos, 2 << 1, 3);   // BFINAL 0, BTYPE 10
            pos += 3;
            put_bits(dw, pos, (unsigned long long)(S.hlit - 257) | (unsigned long long)(S.hdist - 1) << 5 | (unsigned long long)(S.hclen - 4) << 10, 14);
            pos += 14;
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            for (int k = 0; k < S.hclen; k++, pos += 3) put_bits(dw, pos, S.clen[order[k]], 3);
            for (int k = 0; k < S.ncl; k++) {
                const int sym = S.cl_sym[k] & 31, x = S.cl_sym[k] >> 5, xb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
                put_bits(dw, pos, S.ccode[sym] | (unsigned long long)x << S.clen[sym], S.clen[sym] + xb);
                pos += S.clen[sym] + xb;
            }
        }
        // tokens: one per lane per round, positions by an exclusive scan with a running base
        unsigned long long base = S.hbits;
        for (int k0 = 0; k0 < ntok; k0 += kDefThreads) {
            const int k = k0 + t;
            int n = 0;
            unsigned long long v = 0;
            if (k < ntok) v = token_bits(M[s0 + k], S, &n);
            unsigned long long inc = (unsigned long long)n;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long u = __shfl_up(inc, off, 64);
                if ((t & 63) >= off) inc += u;
            }
            __syncthreads();
            if ((t & 63) == 63) S.wsum2[t >> 6] = inc;
            __syncthreads();
            unsigned long long pre = 0, all = 0;
            for (int wv = 0; wv < kDefThreads / 64; wv++) {
                if (wv < (t >> 6)) pre += S.wsum2[wv];
                all += S.wsum2[wv];
            }
            if (k < ntok) put_bits(dw, base + pre + inc - n, v, n);
            base += all;
        }
        if (t == 0) {
            put_bits(dw, base, S.lcode[256], S.llen[256]);
            base += S.llen[256];
            put_bits(dw, base, last ? 1 : 0, 3);   // the empty stored block: BFINAL, BTYPE 00, then byte aligned
            base += 3;
            put_bits(dw, ((base + 7) / 8) * 8 + 16, 0xFFFF, 16);
        }
    }
    __threadfence();
    __syncthreads();

    // ---- 5. the chunk: length, type, CRC-32 of type + data (per-lane raw CRCs shifted into place), and the Adler sums of the segment
    if (t == 0) {
        o[0] = (uint8_t)(dlen >> 24);
        o[1] = (uint8_t)(dlen >> 16);
        o[2] = (uint8_t)(dlen >> 8);
        o[3] = (uint8_t)dlen;
        o[4] = 'I'; o[5] = 'D'; o[6] = 'A'; o[7] = 'T';
    }
    __threadfence();
    __syncthreads();
    const size_t cn = dlen + 4, per = (cn + kDefThreads - 1) / kDefThreads;
    const size_t b0 = min(cn, per * t), b1 = min(cn, b0 + per);
    uint32_t c = 0;
    for (size_t q = b0; q < b1; q++) {
        const uint32_t wd = __hip_atomic_load((const uint32_t *)(o + 4) + (q >> 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t byte = (wd >> (8 * (q & 3))) & 0xFF;
        c = c_png_crc.crc[(c ^ byte) & 0xFF] ^ (c >> 8);
    }
    // contribution of this lane's range: shifted by the bytes after it; the initial ~0 state shifted by all of them
    const unsigned long long contrib = b1 > b0 ? crc_shift(c, (uint32_t)(cn - b1), c_png_crc.x2n) : 0;
    unsigned long long x = contrib;
    for (int off = 32; off > 0; off >>= 1) x ^= __shfl_xor(x, off, 64);
    __syncthreads();
    if ((t & 63) == 0) S.wsum[t >> 6] = x;
    __syncthreads();
    if (t == 0) {
        uint32_t crc = crc_shift(0xFFFFFFFFu, (uint32_t)cn, c_png_crc.x2n);
        for (int i = 0; i < kDefThreads / 64; i++) crc ^= (uint32_t)S.wsum[i];
        crc = ~crc;
        uint8_t *cp = o + 8 + dlen;
        cp[0] = (uint8_t)(crc >> 24);
        cp[1] = (uint8_t)(crc >> 16);
        cp[2] = (uint8_t)(crc >> 8);
        cp[3] = (uint8_t)crc;
        lens[blockIdx.x] = (uint32_t)(dlen + 12);
    }
    const uint32_t per2 = (L + kDefThreads - 1) / kDefThreads, a0 = min(L, per2 * t), a1 = min(L, a0 + per2);
    unsigned long long sa = 0, sb = 0;
    for (uint32_t q = a0; q < a1; q++) {
        const uint32_t byte = data[s0 + q];
        sa += byte;
        sb += (unsigned long long)(a1 - q) * byte;
    }
    sb += (unsigned long long)(L - a1) * sa;
    const unsigned long long A = block_sum(sa, S.wsum), B = block_sum(sb, S.wsum2);
    if (t == 0) {
        adler[2 * blockIdx.x] = (uint32_t)(A % 65521);
        adler[2 * blockIdx.x + 1] = (uint32_t)(B % 65521);
    }
