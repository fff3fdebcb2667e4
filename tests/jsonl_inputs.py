"""Builders of the JSONL buffers that tests/test_jsonl_cpu.py and tests/test_jsonl_gpu.py share. ``test_jsonl_cpu.py``
checks them against ``json.loads``; the expected arrays always come from ``jsonl_restatement.parse`` on the very bytes."""
import itertools

import numpy as np

TYPE_NAMES = ('clicks', 'carts', 'orders')
KEY_ORDERS = tuple(itertools.permutations((0, 1, 2)))        # positions of aid, ts, type
TS0 = 1659304800025                                          # the dataset's first stamp, milliseconds

# named spellings of the punctuation: (after '{' / '[', around ':', around ',', before '}' / ']', line end)
STYLES = {
    'dataset': ('', '', '', '', '\n'),                       # the files' own form, DataFrame.to_json(lines=True)
    'dumps': ('', (' ', 1), (' ', 1), '', '\n'),             # json.dumps' default ", " and ": "
    'spaces': (' ', ' ', ' ', ' ', ' \n'),
    'tabs': ('\t', '\t', '\t', '\t', '\t\n'),
    'cr': ('\r', '\r', '\r', '\r', '\r\n'),
    'crlf': ('', '', '', '', '\r\n'),
}


def _around(spec, ch):
    if isinstance(spec, tuple):                              # (ws, 1): after the character only
        return ch + spec[0]
    return spec + ch + spec


def event(aid, ts, typ, order=(0, 1, 2), style='dataset'):
    inner, colon, comma, close, _ = STYLES[style]
    members = [f'"aid"{_around(colon, ":")}{aid}', f'"ts"{_around(colon, ":")}{ts}',
               f'"type"{_around(colon, ":")}"{TYPE_NAMES[typ]}"']
    return '{' + inner + _around(comma, ',').join(members[k] for k in order) + close + '}'


def line(session, events, style='dataset', orders=None, newline=True):
    """One session line as bytes. ``events``: (aid, ts, type code) triples; ``orders``: a key order per event."""
    inner, colon, comma, close, end = STYLES[style]
    evs = [event(a, t, y, orders[i % len(orders)] if orders else (0, 1, 2), style) for i, (a, t, y) in enumerate(events)]
    body = ('{' + inner + f'"session"{_around(colon, ":")}{session}' + _around(comma, ',') + f'"events"{_around(colon, ":")}['
            + inner + _around(comma, ',').join(evs) + (close if evs else '') + ']' + close + '}')
    return (body + (end if newline else end[:-1])).encode('ascii')


def sessions(seed, n, max_events=12, first=0):
    """``n`` random sessions: (session id, [(aid, ts, type code), ...]) with 1 .. max_events events, stamps in milliseconds."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n):
        k = int(rng.integers(1, max_events + 1))
        t = TS0 + np.cumsum(rng.integers(0, 90_000, k))
        out.append((first + s, [(int(rng.integers(0, 1_855_603)), int(t[i]), int(rng.integers(0, 3))) for i in range(k)]))
    return out


def buffer(sess, style='dataset', orders=None, last_newline=True):
    parts = [line(s, ev, style, orders) for s, ev in sess]
    if parts and not last_newline:
        parts[-1] = parts[-1].rstrip(b'\n')
    return b''.join(parts)


GOOD = line(7, [(11, TS0, 0), (12, TS0 + 5, 1)])            # the 200 good lines of the refusal cases are copies of this one


def exact_size(n_bytes, seed=1):
    """A valid buffer of exactly ``n_bytes`` bytes: random sessions, then empty lines."""
    out, total, s = [], 0, 0
    for sid, ev in sessions(seed, 10 ** 6 if n_bytes > 10 ** 6 else max(n_bytes // 60, 4), max_events=6):
        ln = line(sid, ev)
        if total + len(ln) > n_bytes:
            break
        out.append(ln)
        total += len(ln)
        s += 1
    pad = n_bytes - total
    return b''.join(out) + b'\n' * pad


def slide(lead_blanks, first_len):
    """Two lines: the first followed by empty lines up to ``first_len`` bytes, the second with
    ``lead_blanks`` leading blanks, a 32-byte header and 50-byte events -- as ``lead_blanks`` runs over 0 .. 95 a boundary at
    ``first_len + 96`` falls on every byte of the header and of the first event."""
    first = line(1, [(1, TS0, 0)])
    first = first + b'\n' * (first_len - len(first))
    ev = [(1_000_000 + i, TS0 + i, i % 3) for i in range(4)]
    second = b' ' * lead_blanks + line(4_000_000_000, ev)
    assert len(first) == first_len
    return first + second


# every violation class of the spec: name -> one bad line (no newline)
def _bad_lines():
    e = '{"aid":1,"ts":2,"type":"clicks"}'
    wrap = lambda body: ('{"session":5,"events":[' + body + ']}').encode()
    bad = {
        'sign': wrap('{"aid":-1,"ts":2,"type":"clicks"}'),
        'plus': wrap('{"aid":+1,"ts":2,"type":"clicks"}'),
        'fraction': wrap('{"aid":1.0,"ts":2,"type":"clicks"}'),
        'exponent': wrap('{"aid":1,"ts":2e3,"type":"clicks"}'),
        'leading_zero': wrap('{"aid":01,"ts":2,"type":"clicks"}'),
        'session_leading_zero': b'{"session":007,"events":[]}',
        'aid_overflow': wrap('{"aid":4294967296,"ts":2,"type":"clicks"}'),
        'session_overflow': b'{"session":4294967296,"events":[]}',
        'ts_overflow': wrap('{"aid":1,"ts":9223372036854775808,"type":"clicks"}'),
        'ts_huge': wrap('{"aid":1,"ts":' + '9' * 40 + ',"type":"clicks"}'),
        'escape_key': wrap('{"a\\u0069d":1,"ts":2,"type":"clicks"}'),
        'escape_type': wrap('{"aid":1,"ts":2,"type":"click\\u0073"}'),
        'other_key': wrap('{"aid":1,"ts":2,"kind":"clicks"}'),
        'fourth_key': wrap('{"aid":1,"ts":2,"type":"clicks","x":1}'),
        'top_level_extra_key': b'{"session":5,"events":[],"x":1}',
        'swapped_top_level': b'{"events":[],"session":5}',
        'type_string': wrap('{"aid":1,"ts":2,"type":"click"}'),
        'type_number': wrap('{"aid":1,"ts":2,"type":0}'),
        'aid_string': wrap('{"aid":"1","ts":2,"type":"clicks"}'),
        'upper_case': wrap('{"aid":1,"ts":2,"type":"Clicks"}'),
        'high_byte': b'{"session":5,"events":[]}\xc3\xa9',
        'high_byte_ws': b'{"session":5,\xe2\x80\x8b"events":[]}',
        'bom': b'\xef\xbb\xbf{"session":5,"events":[]}',
        'nul_byte': b'{"session":5,"events":[]}\x00',
        'form_feed_ws': b'{"session":5,\x0c"events":[]}',
        'duplicate_key': wrap('{"aid":1,"aid":2,"type":"clicks"}'),
        'missing_key': wrap('{"aid":1,"ts":2}'),
        'missing_session': b'{"events":[]}',
        'trailing_comma_events': wrap(e + ','),
        'trailing_comma_members': wrap('{"aid":1,"ts":2,"type":"clicks",}'),
        'trailing_comma_top': b'{"session":5,"events":[],}',
        'missing_comma_events': wrap(e + e),
        'missing_comma_members': wrap('{"aid":1 "ts":2,"type":"clicks"}'),
        'leading_comma': wrap(',' + e),
        'nested_object': wrap('{"aid":{"x":1},"ts":2,"type":"clicks"}'),
        'nested_array': wrap('[' + e + ']'),
        'nested_event': wrap('{' + e + '}'),
        'extra_close': wrap(e) + b'}',
        'two_objects': b'{"session":5,"events":[]}{"session":6,"events":[]}',
        'text_after': b'{"session":5,"events":[]} x',
        'text_before': b'x {"session":5,"events":[]}',
        'bare_word': b'null',
        'single_quotes': b"{'session':5,'events':[]}",
        'unclosed': b'{"session":5,"events":[' + e.encode(),
        'events_object': b'{"session":5,"events":{}}',
        'piece_257_event': wrap('{"aid":1,' + ' ' * (257 - len(e + ']}')) + '"ts":2,"type":"clicks"}'),
        'piece_257_header': b'{"session":5,' + b' ' * (257 - len(b'{"session":5,"events":[]}')) + b'"events":[]}',
        'piece_257_lead': b' ' * 257 + b'{"session":5,"events":[]}',
        'piece_257_blank': b' ' * 257,
        'ws_1000_in_event': wrap('{"aid":1,' + ' ' * 1000 + '"ts":2,"type":"clicks"}'),
    }
    return bad


BAD_LINES = _bad_lines()

# the longest legal pieces: accepted
LONG_OK = {
    'piece_256_event': ('{"session":5,"events":[{"aid":1,' + ' ' * (256 - len('{"aid":1,"ts":2,"type":"clicks"}]}'))
                        + '"ts":2,"type":"clicks"}]}').encode(),
    'piece_256_header': b'{"session":5,' + b' ' * (256 - len(b'{"session":5,"events":[]}')) + b'"events":[]}',
    'piece_256_lead': b' ' * 256 + b'{"session":5,"events":[]}',
    'piece_256_blank': b' ' * 256,
}


def with_bad_line(bad, where, n_good=200):
    """``n_good`` good lines and ``bad`` as line number ``where`` (1-based); returns the buffer."""
    lines = [GOOD] * n_good
    lines.insert(where - 1, bad + b'\n')
    return b''.join(lines)


def truncations():
    """A buffer whose last line is cut at every byte of its last event (the complete line is not among them)."""
    head = GOOD * 3
    last = line(9, [(1, TS0, 0), (22, TS0 + 1, 2)], newline=False)
    start = last.rindex(b'{')
    return [head + last[:k] for k in range(start, len(last))]


def acceptance_corpus():
    """name -> buffer that SPEC-JSONL accepts."""
    s = sessions(3, 40)
    out = {f'style_{name}': buffer(s, name) for name in STYLES}
    out['key_orders'] = buffer(s, 'dataset', orders=KEY_ORDERS)
    out['key_orders_dumps'] = buffer(s, 'dumps', orders=KEY_ORDERS)
    out['no_last_newline'] = buffer(s, last_newline=False)
    out['empty'] = b''
    out['one_line'] = buffer(s[:1])
    out['blank_only'] = b'\n \n\t\r\n\n   '
    out['empty_events'] = (line(1, []) + buffer(s[:3]) + line(2, [], 'spaces') + buffer(s[3:5]) + line(3, [], 'dataset', newline=False))
    out['limits'] = b''.join([line(0, [(0, 0, 0), (4294967295, TS0, 1), (5, 9223372036854775807, 2)]),
                              line(4294967295, [(4294967295, 0, 2)])])
    out['blank_between'] = b'\n'.join([GOOD.rstrip(b'\n'), b'', b' \t', GOOD.rstrip(b'\n'), b'\r', b''])
    for name, ln in LONG_OK.items():
        out[name] = GOOD + ln + b'\n' + GOOD
    # 2,048 one-byte pieces in a tile of 4,096 bytes: more than the kernel's piece list takes in one round
    out['many_pieces'] = b' \n' * 3000 + GOOD + b'\t\n' * 1500 + b'\n' * 700 + GOOD[:-1]
    return out


def many_pieces_bad():
    """(buffer, number of its only bad line): the bad line follows tiles of one-byte pieces."""
    return b' \n' * 3000 + GOOD + b'\r\n' * 2100 + BAD_LINES['type_string'] + b'\n' + GOOD, 5102


def mutation_corpus(n=300, seed=20221101, lines=40):
    """``n`` buffers of about ``lines`` lines with one substituted, deleted or inserted byte each (fixed seed). Most
    are violations, some stay valid (a digit for a digit, a blank more); the expectation is the restatement's verdict."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b'{}[]":,0123456789 \t\r\n-+.eE\\aidtsypclkorn\x00\xef\x80', dtype=np.uint8)
    styles = list(STYLES)
    out = []
    for i in range(n):
        base = bytearray(buffer(sessions(1000 + i, lines, max_events=5), styles[i % len(styles)], orders=KEY_ORDERS,
                                last_newline=bool(i % 7)))
        pos = int(rng.integers(0, len(base)))
        op = i % 3
        if op == 0:
            base[pos] = int(alphabet[rng.integers(0, len(alphabet))])
        elif op == 1:
            del base[pos]
        else:
            base.insert(pos, int(alphabet[rng.integers(0, len(alphabet))]))
        out.append(bytes(base))
    return out


def halo_slide(j, tile, piece=256):
    """Empty lines, then a line whose single event piece is ``piece`` bytes long and starts at byte ``tile - 1 - j``: with
    ``piece`` 256 its last byte is the workgroup's halo byte ``255 - j`` and the newline the parser must see follows it;
    two good lines follow."""
    head = b'{"session":5,"events":['
    tail = b'"ts":2,"type":"clicks"}]}'
    ev = b'{"aid":1,' + b' ' * (piece - len(b'{"aid":1,') - len(tail)) + tail
    lead = tile - 1 - j - len(head)
    return b'\n' * lead + head + ev + b'\n' + GOOD * 2


def long_line(n_events=500):
    return line(77, [(i * 3571 % 1_855_603, TS0 + 1000 * i, i % 3) for i in range(n_events)], orders=KEY_ORDERS)
