"""SPEC-DEFLATE (include/otto_deflate.h) restated in plain Python, written from the header's text: a byte string and
``block_bytes`` -> the bytes of the concatenated gzip members. Slow and sequential on purpose; the device kernels
(csrc/otto_deflate.hip) must produce these bytes exactly."""

BLOCK_MAX = 65536          # OTTO_DEFLATE_BLOCK_MAX
MIN_MATCH = 6              # OTTO_DEFLATE_MIN_MATCH
MAX_MATCH = 258
MAX_DIST = 32768
HASH_BYTES = 6             # OTTO_DEFLATE_HASH_BYTES
HASH_BITS = 12             # OTTO_DEFLATE_HASH_BITS
BATCH = 64                 # OTTO_DEFLATE_BATCH
HASH_MUL = 0x9E3779B97F4A7C15
GZIP_HEADER = bytes([0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0, 0xFF])
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

# RFC 1951 section 3.2.5: base value and extra bits of the length symbols 257..285 and of the distance symbols 0..29
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def _crc_table():
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0xEDB88320 if c & 1 else c >> 1
        table.append(c)
    return table


_CRC = _crc_table()


def crc32(data):
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3..258"""
    if length == 258:
        return 285, 0, 0
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


def _common(x, a, b, limit):
    n = 0
    while n < limit and x[a + n] == x[b + n]:
        n += 1
    return n


def tokens(x):
    """The match finder and the greedy selection of one block: a list of ints (a literal byte) and (length, distance)."""
    n = len(x)
    table = [-1] * (1 << HASH_BITS)
    out = []
    p = 0                                                    # the next position the greedy selection stands on
    for base in range(0, n, BATCH):
        top = min(base + BATCH, n)
        slot, seen = {}, {}
        for q in range(base, top):                           # what the batch sees of the table: earlier batches only
            if q + HASH_BYTES <= n:
                v = int.from_bytes(x[q:q + HASH_BYTES], 'little')
                slot[q] = ((v * HASH_MUL) & 0xFFFFFFFFFFFFFFFF) >> (64 - HASH_BITS)
                seen[q] = table[slot[q]]
        for q, s in slot.items():                            # ascending: the batch's last position of a slot stays
            table[s] = q
        while p < top:
            limit = min(MAX_MATCH, n - p)
            length, dist = 0, 0
            if p >= 1:
                length, dist = _common(x, p - 1, p, limit), 1
            c = seen.get(p, -1)
            if c >= 0 and p - c <= MAX_DIST:
                l2 = _common(x, c, p, limit)
                if l2 > length:                              # a tie stays with distance 1
                    length, dist = l2, p - c
            if length >= MIN_MATCH:
                out.append((length, dist))
                p += length
            else:
                out.append(x[p])
                p += 1
    return out


def huff_lengths(counts, limit):
    """Code lengths of the symbols with a count > 0 (0 for the others), none above ``limit``."""
    n = len(counts)
    used = [s for s in range(n) if counts[s] > 0]
    lengths = [0] * n
    if len(used) == 1:
        lengths[used[0]] = 1
    if len(used) < 2:
        return lengths
    c = list(counts)
    while True:
        order = sorted(used, key=lambda s: (c[s], s))
        m = len(order)
        leaf_parent, node_w, node_parent = [0] * m, [], [0] * (m - 1)
        li = ni = 0

        def take(j):
            nonlocal li, ni
            # the lighter of the two queue heads; the leaf on a tie
            if li < m and (ni >= len(node_w) or c[order[li]] <= node_w[ni]):
                leaf_parent[li] = j
                li += 1
                return c[order[li - 1]]
            node_parent[ni] = j
            ni += 1
            return node_w[ni - 1]

        for j in range(m - 1):
            a = take(j)
            b = take(j)
            node_w.append(a + b)
        depth = [0] * (m - 1)
        for j in range(m - 3, -1, -1):
            depth[j] = depth[node_parent[j]] + 1
        for i, s in enumerate(order):
            lengths[s] = depth[leaf_parent[i]] + 1
        if max(lengths) <= limit:
            return lengths
        for s in used:
            c[s] = (c[s] + 1) >> 1


def canonical_codes(lengths):
    """RFC 1951 section 3.2.2"""
    top = max(lengths) if lengths else 0
    bl_count = [0] * (top + 2)
    for l in lengths:
        if l:
            bl_count[l] += 1
    code, next_code = 0, [0] * (top + 2)
    for bits in range(1, top + 1):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = next_code[l]
            next_code[l] += 1
    return codes


def run_length_tokens(seq):
    """The joint sequence of code lengths -> (symbol, extra bits, extra value)"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        r = 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            t = min(r, 138)
            out.append((18, 7, t - 11))
        elif v == 0 and r >= 3:
            t = r
            out.append((17, 3, t - 3))
        elif v != 0 and i > 0 and seq[i - 1] == v and r >= 3:
            t = min(r, 6)
            out.append((16, 2, t - 3))
        else:
            t = 1
            out.append((v, 0, 0))
        i += t
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, value, bits):
        """``bits`` bits of ``value``, least significant first"""
        self.acc |= (value & ((1 << bits) - 1)) << self.n
        self.n += bits
        self.total += bits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, bits):
        """a Huffman code: most significant bit first"""
        self.put(int(format(code, f'0{bits}b')[::-1], 2) if bits else 0, bits)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b'')


def plan(x):
    """Everything SPEC-DEFLATE derives from one non-empty block before it writes: a dict."""
    toks = tokens(x)
    ll, dd = [0] * 286, [0] * 30
    for t in toks:
        if isinstance(t, tuple):
            ll[length_symbol(t[0])[0]] += 1
            dd[dist_symbol(t[1])[0]] += 1
        else:
            ll[t] += 1
    ll[256] = 1
    ll_len, d_len = huff_lengths(ll, 15), huff_lengths(dd, 15)
    hlit = max(s for s in range(286) if ll_len[s]) + 1
    hlit = max(hlit, 257)
    hdist = max([s for s in range(30) if d_len[s]] or [0]) + 1
    rl = run_length_tokens(ll_len[:hlit] + d_len[:hdist])
    cl = [0] * 19
    for s, _, _ in rl:
        cl[s] += 1
    cl_len = huff_lengths(cl, 7)
    hclen = max(max(i for i in range(19) if cl_len[CLEN_ORDER[i]]) + 1, 4)
    bits = 3 + 5 + 5 + 4 + 3 * hclen + sum(cl_len[s] + e for s, e, _ in rl)
    bits += sum(ll[s] * (ll_len[s] + (LEN_EXTRA[s - 257] if s > 256 else 0)) for s in range(286))
    bits += sum(dd[s] * (d_len[s] + DIST_EXTRA[s]) for s in range(30))
    n = len(x)
    stored = n + 5 * (2 if n > 65535 else 1)
    return dict(tokens=toks, ll=ll, dd=dd, ll_len=ll_len, d_len=d_len, hlit=hlit, hdist=hdist, rl=rl, cl_len=cl_len, hclen=hclen,
                bits=bits, dynamic_bytes=(bits + 7) // 8, stored_bytes=stored, dynamic=(bits + 7) // 8 < stored)


def deflate_stream(x):
    n = len(x)
    if n == 0:
        return bytes([0x03, 0x00])
    p = plan(x)
    if not p['dynamic']:
        out = bytearray()
        for lo in range(0, n, 65535):
            m = min(65535, n - lo)
            out += bytes([1 if lo + m == n else 0, m & 0xFF, m >> 8, (m & 0xFF) ^ 0xFF, (m >> 8) ^ 0xFF]) + x[lo:lo + m]
        return bytes(out)
    w = _Bits()
    w.put(1, 1)
    w.put(2, 2)
    w.put(p['hlit'] - 257, 5)
    w.put(p['hdist'] - 1, 5)
    w.put(p['hclen'] - 4, 4)
    for i in range(p['hclen']):
        w.put(p['cl_len'][CLEN_ORDER[i]], 3)
    cl_code = canonical_codes(p['cl_len'])
    for s, e, v in p['rl']:
        w.code(cl_code[s], p['cl_len'][s])
        w.put(v, e)
    ll_code, d_code = canonical_codes(p['ll_len']), canonical_codes(p['d_len'])
    for t in p['tokens']:
        if isinstance(t, tuple):
            s, e, v = length_symbol(t[0])
            w.code(ll_code[s], p['ll_len'][s])
            w.put(v, e)
            s, e, v = dist_symbol(t[1])
            w.code(d_code[s], p['d_len'][s])
            w.put(v, e)
        else:
            w.code(ll_code[t], p['ll_len'][t])
    w.code(ll_code[256], p['ll_len'][256])
    assert w.total == p['bits']
    return w.bytes()


def member(x):
    x = bytes(x)
    assert len(x) <= BLOCK_MAX
    return GZIP_HEADER + deflate_stream(x) + crc32(x).to_bytes(4, 'little') + len(x).to_bytes(4, 'little')


def gzip_members(data, block_bytes=BLOCK_MAX):
    data = bytes(data)
    if not 1 <= block_bytes <= BLOCK_MAX:
        raise ValueError('block_bytes must be in [1, 65536]')
    if not data:
        return member(b'')
    return b''.join(member(data[lo:lo + block_bytes]) for lo in range(0, len(data), block_bytes))


def compressed_bound(n, block_bytes=BLOCK_MAX):
    """every member in the stored form"""
    blocks = max(1, -(-n // block_bytes))
    return n + blocks * (18 + (10 if block_bytes > 65535 else 5))
