// mpb_crc_lane.inc -- what ONE LANE of the device CRC-32 does (mpb_crc_kernels.hip: k_bgzf_crc32), with no wave intrinsic in it, so
// that a host program runs the same text with checked loads (tests/helpers/crc_lane_check.cpp).  The includer defines
//     CRC_FN                       the function qualifier (__device__ __forceinline__ / static inline)
//     CRC_CONST                    the qualifier of the constant table (__device__ static const / static const)
//     CrcWord                      four 32-bit words: 16 text bytes, little-endian
//     CRC_LDW(text, p)             the 16 bytes at byte p of the text, asked for only when p is a multiple of 16 and the whole
//                                  word lies inside the lane's slice (so inside the range, so inside the text)
//     CRC_LDB(text, p)             byte p of the text, asked for only inside the lane's slice
//     CRC_TAB(tab, k, i)           word i of table k (tab[k * 256 + i]), 0 <= k < 4, 0 <= i < 256
// RFC 1952's CRC-32, reflected polynomial 0xEDB88320.  With reg(M, I) the register after the bytes M from the start value I
// (no final inversion), crc32(M) = reg(M, 0xFFFFFFFF) ^ 0xFFFFFFFF and, for M = A || B,
//     reg(A || B, I) = reg(A, I) (x) x^(8 |B|)  ^  reg(B, 0)                     ((x): multiplication modulo the polynomial)
// so a range is cut into slices of CRC_SLICE bytes COUNTED FROM ITS END, lane j takes the j-th of them (the last lane that holds
// bytes takes the range's short head and alone starts from 0xFFFFFFFF; for an empty range that is lane 0, with no bytes), every
// lane multiplies its register by x^(8 CRC_SLICE j) -- the bytes that follow its slice -- and the xor over the wave, inverted, is
// the CRC.  A lane reads its slice and nothing else: single bytes up to the first multiple of 16, whole aligned 16-byte words,
// single bytes again.  Every loop runs over the slice or the 32 bits of a factor.

#define CRC_POLY      0xedb88320u
#define CRC_SLICE     1024                        // bytes of a lane's slice
#define CRC_LANES     64                          // one wave per range
#define CRC_RANGE_MAX (CRC_SLICE * CRC_LANES)     // 65536: a BGZF member's text at most
#define CRC_BAD_RANGE 1u                          // the marker of a range that failed the kernel's own check (crc 0, nothing read)

#ifndef CRC_START_VALUE
#define CRC_START_VALUE 0xffffffffu               // (the sensitivity builds of the host checker set another)
#endif
#ifndef CRC_FACTOR_OF_LANE
#define CRC_FACTOR_OF_LANE(j) (j)                 // (likewise)
#endif

// x^(8 * CRC_SLICE * j) modulo the polynomial, j = 0 .. 63, bit-reflected as the register is (x^0 = 0x80000000); the host
// checker recomputes every entry by square-and-multiply
CRC_CONST uint32_t crc_slice_factor[CRC_LANES] = {
    0x80000000u, 0x6427800eu, 0x4d47bae0u, 0x6347a4bdu, 0x09fe548fu, 0x923b0526u, 0x552d4042u, 0x63c21244u,
    0x83852d0fu, 0x4d29b1c7u, 0x4e2f9ac3u, 0x4ccd837bu, 0xe4b54665u, 0x7da28b5cu, 0x96a2a2f2u, 0x4a5348d2u,
    0x30362f1au, 0x674e5450u, 0x090e1204u, 0x8838d750u, 0x668145e1u, 0x0f6b1269u, 0x80c95e61u, 0x8fc4160bu,
    0xf27674adu, 0x0d141499u, 0x70d4f062u, 0xebe4475eu, 0xb8c9f94bu, 0xad5e8b5au, 0x3f2d3b68u, 0xd38c9653u,
    0x7b5a9cc3u, 0x675f7815u, 0x5307d760u, 0xe3d20a6au, 0x866744b2u, 0xac24b8aau, 0xecfa96e2u, 0x4577ee9au,
    0xc99622b9u, 0x54716e20u, 0x5773aa46u, 0x5d77e65cu, 0xafe90854u, 0x5bc32d87u, 0xb11d39f9u, 0xad989cddu,
    0xec735ceau, 0xde02da1du, 0xdec9f6f0u, 0xfdbc90a8u, 0xefe9d761u, 0x549a7413u, 0x4f99e7a4u, 0x690be0f7u,
    0x0f9f0002u, 0x39e53f8cu, 0xb752dd13u, 0xeaff9ca5u, 0xf014301eu, 0xa7e95db6u, 0xa895beecu, 0xd2ba56f9u};

// the range the kernel was given, checked against the text it was given
CRC_FN bool crc_range_ok(int64_t off, int64_t len, int64_t text_bytes)
{
    return off >= 0 && len >= 0 && len <= CRC_RANGE_MAX && off <= text_bytes && len <= text_bytes - off;
}

// Entry i of the four tables: table k holds the register after byte i and k zero bytes, so that four bytes are one step
// (slicing by four).  out[k] = tab[k][i].
CRC_FN void crc_table_entry(uint32_t i, uint32_t out[4])
{
    uint32_t c = i;
    for (int s = 0; s < 32; s++) {
        c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
        if ((s & 7) == 7) out[s >> 3] = c;
    }
}

// a (x) b modulo the polynomial (32 steps of shift and xor)
CRC_FN uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}

struct CrcLane { int64_t p, end; uint32_t c; };

// lane j of the wave that owns the range [off, off + len): its slice [p, end) and its start value
CRC_FN void crc_lane_begin(int64_t off, int64_t len, int j, CrcLane *L)
{
    const int64_t stop = off + len;
    const int64_t slices = (len + CRC_SLICE - 1) / CRC_SLICE;
    const int64_t first = slices > 0 ? slices - 1 : 0;       // the lane that holds the range's first byte (lane 0: an empty range)
    int64_t end = stop - (int64_t)CRC_SLICE * j, p = end - CRC_SLICE;
    if (end < off) end = off;
    if (p < off) p = off;
    L->p = p; L->end = end;
    L->c = j == first ? CRC_START_VALUE : 0u;
}

CRC_FN uint32_t crc_byte(const uint32_t *tab, uint32_t c, uint32_t b)
{
    return CRC_TAB(tab, 0, (c ^ b) & 0xffu) ^ (c >> 8);
}

CRC_FN uint32_t crc_word(const uint32_t *tab, uint32_t c, uint32_t w)
{
    c ^= w;
    return CRC_TAB(tab, 3, c & 0xffu) ^ CRC_TAB(tab, 2, (c >> 8) & 0xffu) ^ CRC_TAB(tab, 1, (c >> 16) & 0xffu) ^ CRC_TAB(tab, 0, c >> 24);
}

// One step of the lane: a byte, or an aligned 16-byte word that lies inside the slice.  false: the slice is done (nothing read).
CRC_FN bool crc_lane_step(const uint8_t *text, const uint32_t *tab, CrcLane *L)
{
    if (L->p >= L->end) return false;
    if ((L->p & 15) == 0 && L->end - L->p >= 16) {
        const CrcWord v = CRC_LDW(text, L->p);
        uint32_t c = L->c;
        c = crc_word(tab, c, v.x); c = crc_word(tab, c, v.y); c = crc_word(tab, c, v.z); c = crc_word(tab, c, v.w);
        L->c = c; L->p += 16;
    } else {
        L->c = crc_byte(tab, L->c, CRC_LDB(text, L->p));
        L->p += 1;
    }
    return true;
}

// what the lane gives to the wave's xor: its register moved over the bytes that follow its slice
CRC_FN uint32_t crc_lane_end(const CrcLane *L, int j)
{
    return crc_mulmod(L->c, crc_slice_factor[CRC_FACTOR_OF_LANE(j)]);
}
