"""Plain Python/numpy restatement of the reference's string spaces (data type 3).

leven: levenshtein (src/distcomp_edist.cc), unit-cost edit distance over bytes, on objects holding the string's bytes.
bit_hamming: the object is the parsed 0/1 values packed into uint32 words (Binarize, include/permutation_utils.h),
followed by the element count as a trailing word (include/space/space_bit_vector.h:156-200); the distance is the
popcount of XOR over every word but the trailing one (BitHamming, include/distcomp.h:241-250)."""
import numpy as np

LABEL_PREFIX = b"label:"
_SPACE = b" \t\n\v\f\r"


class ParseError(ValueError):
    pass


def _extract_label(line):
    """Object::extractLabel: a leading 'label:<int><whitespace>' is removed (a malformed one is an error)."""
    if len(line) > len(LABEL_PREFIX) + 1 and line.startswith(LABEL_PREFIX):
        p = next((i for i in range(len(LABEL_PREFIX), len(line)) if line[i] in _SPACE), -1)
        if p < 0:
            raise ParseError("no space after the label")
        num = line[len(LABEL_PREFIX):p]
        try:
            int(num.decode("ascii"))
        except (UnicodeDecodeError, ValueError):
            raise ParseError("bad label") from None
        j = p
        while j < len(line) and line[j] in _SPACE:
            j += 1
        return line[j:]
    return line


def _strtol_all(s):
    """ReadVecDataEfficiently<int>: strtol repeatedly (leading whitespace, optional sign, decimal digits) until it
    parses nothing; the rest of the line is ignored."""
    out, i, n = [], 0, len(s)
    while True:
        j = i
        while j < n and s[j] in _SPACE:
            j += 1
        k = j
        if k < n and s[k] in b"+-":
            k += 1
        d = k
        while d < n and 48 <= s[d] <= 57:
            d += 1
        if d == k:
            return out
        v = int(s[j:d])
        if not -2**31 <= v < 2**31:
            raise ParseError("value out of range")
        out.append(v)
        i = d


def parse_bits(s):
    """The text of one bit_hamming object -> list of 0/1 values (ReadBitMaskVect)."""
    if isinstance(s, str):
        s = s.encode()
    s = s.split(b"\0", 1)[0]
    s = _extract_label(s)
    s = s.replace(b",", b" ").replace(b":", b" ")          # ReplaceSomePunct
    v = _strtol_all(s)
    if any(x not in (0, 1) for x in v):
        raise ParseError("only zeros and ones are allowed")
    return v


def bit_object(s):
    """-> uint32 words of the reference's object: packed bits, then the bit count."""
    v = parse_bits(s)
    w = np.zeros((len(v) + 31) // 32 + 1, np.uint32)
    for i, b in enumerate(v):
        if b:
            w[i // 32] |= np.uint32(1 << (i % 32))
    w[-1] = len(v)
    return w


def bit_hamming(a, b):
    """a, b: objects from bit_object."""
    x = np.bitwise_xor(a[:-1], b[:-1])
    return int(sum(bin(int(t)).count("1") for t in x))


def levenshtein(a, b):
    if isinstance(a, str):
        a = a.encode()
    if isinstance(b, str):
        b = b.encode()
    if len(a) > len(b):
        a, b = b, a
    prev = np.arange(len(a) + 1, dtype=np.int64)
    if len(a) == 0:
        return len(b)
    av = np.frombuffer(a, np.uint8)
    for j, c in enumerate(b):
        cur = np.empty_like(prev)
        cur[0] = j + 1
        sub = prev[:-1] + (av != c)
        ins = prev[1:] + 1
        best = np.minimum(sub, ins)
        # cur[i] = min(best[i-1], cur[i-1] + 1): a running minimum along the column
        run = best - np.arange(1, len(a) + 1)
        run = np.minimum.accumulate(np.minimum(run, cur[0]))
        cur[1:] = run + np.arange(1, len(a) + 1)
        prev = cur
    return int(prev[-1])


def knn(dist_row_query, n, k):
    """Exact k-NN of one query in (distance, position) order: dist_row_query(i) -> int."""
    d = np.array([dist_row_query(i) for i in range(n)], np.int64)
    order = np.lexsort((np.arange(n), d))[:k]
    return order, d[order]


# ---- HNSW search with searchMethod_ = 0 (src/method/hnsw.cc:1078-1290) ------------------------------------------------
# Equal distances are ordered by position: every set is keyed (distance, position).  links(node, level) -> neighbour
# positions; dist(node) -> int distance to the query.
def hnsw_search(links, levels_top, enterpoint, dist, ef, k, old):
    """-> (positions, distances, ndc) of baseSearchAlgorithmOld (old) or baseSearchAlgorithmV1Merge"""
    import heapq
    cur = enterpoint
    curdist = dist(cur)
    ndc = 1
    for lvl in range(levels_top, 0, -1):
        changed = True
        while changed:
            changed = False
            for v in links(cur, lvl):
                d = dist(v)
                ndc += 1
                if d < curdist:
                    curdist, cur, changed = d, v, True
    visited = {cur}
    if not old:
        cap = max(ef, k)
        arr = [[(curdist, cur), False]]
        cur_elem = 0
        while cur_elem < min(len(arr), ef):
            arr[cur_elem][1] = True
            node = arr[cur_elem][0][1]
            cur_elem += 1
            top = arr[-1][0][0]
            buf = []
            for v in links(node, 0):
                if v in visited:
                    continue
                visited.add(v)
                d = dist(v)
                ndc += 1
                if d < top or len(arr) < ef:
                    buf.append((d, v))
            for item in sorted(buf):
                if len(arr) == cap and item >= arr[-1][0]:
                    continue
                if len(arr) == cap:
                    arr.pop()
                pos = 0
                while pos < len(arr) and arr[pos][0] < item:
                    pos += 1
                arr.insert(pos, [item, False])
                cur_elem = min(cur_elem, pos)
            while cur_elem < len(arr) and arr[cur_elem][1]:
                cur_elem += 1
        res = [a[0] for a in arr[:k]]
    else:
        cand = [(curdist, cur)]
        closest = [(-curdist, -cur)]             # max-heap of (distance, position)
        res = [(curdist, cur)]
        while cand:
            if cand[0] > (-closest[0][0], -closest[0][1]):
                break
            _, node = heapq.heappop(cand)
            for v in links(node, 0):
                if v in visited:
                    continue
                visited.add(v)
                d = dist(v)
                ndc += 1
                key = (d, v)
                if key < (-closest[0][0], -closest[0][1]) or len(closest) < ef:
                    res.append(key)
                    res = sorted(res)[:k]
                    heapq.heappush(cand, key)
                    heapq.heappush(closest, (-d, -v))
                    if len(closest) > ef:
                        heapq.heappop(closest)
        res = sorted(res)[:k]
    return [p for _, p in res], [d for d, _ in res], ndc
