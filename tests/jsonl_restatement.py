"""SPEC-JSONL (include/otto_jsonl.h) restated on the host: one compiled ``bytes`` regex per line, a distinct-keys check, the
integer ranges, the piece-length rule and ``json.loads`` for the values. ``parse`` returns the six arrays of
``otto_jsonl_parse`` or raises :class:`Violation` with the 1-based number of the smallest violating line."""
import json
import re

import numpy as np

MAX_PIECE = 256

_WS = rb'[ \t\r]*'
_INT = rb'(?:0|[1-9][0-9]*)'
_MEMBER = (rb'(?:"aid"' + _WS + rb':' + _WS + _INT + rb'|"ts"' + _WS + rb':' + _WS + _INT
           + rb'|"type"' + _WS + rb':' + _WS + rb'"(?:clicks|carts|orders)")')
_EVENT = rb'\{' + _WS + _MEMBER + _WS + rb',' + _WS + _MEMBER + _WS + rb',' + _WS + _MEMBER + _WS + rb'\}'
LINE = re.compile(_WS + rb'\{' + _WS + rb'"session"' + _WS + rb':' + _WS + _INT + _WS + rb',' + _WS + rb'"events"' + _WS + rb':'
                  + _WS + rb'\[' + _WS + rb'(?:' + _EVENT + rb'(?:' + _WS + rb',' + _WS + _EVENT + rb')*' + _WS + rb')?\]' + _WS
                  + rb'\}' + _WS)
_OPEN = re.compile(rb'\{')
TYPES = {'clicks': 0, 'carts': 1, 'orders': 2}


class Violation(ValueError):
    def __init__(self, line, why):
        super().__init__(f'line {line}: {why}')
        self.line = line


def _pairs(items):
    keys = [k for k, _ in items]
    if len(set(keys)) != len(keys):
        raise ValueError('duplicate key')
    return dict(items)


def parse_line(line):
    """One line without its newline -> None (blank) or (session, [(aid, ts, type code), ...]); ValueError on a violation."""
    if not line.strip(b' \t\r'):
        if len(line) > MAX_PIECE:
            raise ValueError('piece too long')
        return None
    if not LINE.fullmatch(line):
        raise ValueError('does not match the grammar')
    # pieces: leading ws | header up to the first event or the line end | each event up to the next one or the line end
    cuts = [0] + [m.start() for m in _OPEN.finditer(line)] + [len(line)]
    if max(b - a for a, b in zip(cuts, cuts[1:])) > MAX_PIECE:
        raise ValueError('piece too long')
    doc = json.loads(line.decode('ascii'), object_pairs_hook=_pairs)
    if doc['session'] > 2 ** 32 - 1:
        raise ValueError('session out of range')
    events = []
    for e in doc['events']:
        if e['aid'] > 2 ** 32 - 1 or e['ts'] > 2 ** 63 - 1:
            raise ValueError('number out of range')
        events.append((e['aid'], e['ts'], TYPES[e['type']]))
    return doc['session'], events


def parse(buf, line0=0):
    """The buffer ``buf`` -> dict of session u32 [E], aid u32 [E], ts i64 [E], type u8 [E], sess_id u32 [S], sess_off i64 [S + 1]."""
    lines = bytes(buf).split(b'\n')
    if lines[-1] == b'':
        lines.pop()                       # the text after the last newline is a line only if there is some
    sess_id, sess_off, session, aid, ts, typ = [], [0], [], [], [], []
    for i, line in enumerate(lines):
        try:
            row = parse_line(line)
        except ValueError as e:
            raise Violation(line0 + i + 1, str(e)) from None
        if row is None:
            continue
        sess_id.append(row[0])
        for a, t, y in row[1]:
            session.append(row[0])
            aid.append(a)
            ts.append(t)
            typ.append(y)
        sess_off.append(len(aid))
    return dict(session=np.array(session, dtype=np.uint32), aid=np.array(aid, dtype=np.uint32), ts=np.array(ts, dtype=np.int64),
                type=np.array(typ, dtype=np.uint8), sess_id=np.array(sess_id, dtype=np.uint32),
                sess_off=np.array(sess_off, dtype=np.int64))


def verdict(buf, line0=0):
    """(None, arrays) where the buffer is accepted, (line, None) where it is refused."""
    try:
        return None, parse(buf, line0)
    except Violation as v:
        return v.line, None


def frame(bufs):
    """The frame the reference's ``create_dataframe`` builds (``dataset_writer_pickle.py:56-63``) from the files' bytes."""
    import pandas as pd
    cols = [parse(b) for b in (bufs if isinstance(bufs, (list, tuple)) else [bufs])]
    cat = lambda k: np.concatenate([c[k] for c in cols])
    return pd.DataFrame({'session': cat('session'), 'aid': cat('aid'), 'ts': cat('ts').astype(np.uint64), 'type': cat('type')})
