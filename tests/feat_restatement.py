"""Plain NumPy / Python restatement of SPEC-FEAT (include/otto_feat.h): the aid table, the session
table and the feature matrix, sequential and in float64 with Python integers for every exact sum. Test infrastructure:
the device tables are compared with this, and this is compared with the recorded output of the reference's two scripts
(tests/golden/feat_golden.npz)."""
import datetime
import math

import numpy as np

AID_COLUMNS = (
    'aid_type_mean', 'aid_hour_mean', 'aid_hour_std', 'aid_day_of_week_mean', 'aid_day_of_week_std', 'aid_ts_ratio',
    'aid_is_session_start_mean', 'aid_is_session_end_mean', 'aid_count_rank_pct', 'aid_day_of_year_nunique_rank_pct',
    'aid_click_count_rank_pct', 'aid_cart_count_rank_pct', 'aid_order_count_rank_pct',
    'aid_click_session_nunique_rank_pct', 'aid_cart_session_nunique_rank_pct', 'aid_order_session_nunique_rank_pct',
    'aid_click_day_of_year_nunique_rank_pct', 'aid_cart_day_of_year_nunique_rank_pct', 'aid_order_day_of_year_nunique_rank_pct',
    'aid_last_week_count_rank_pct', 'aid_last_week_ts_ratio', 'aid_last_week_day_of_week_mean',
    'aid_click_last_week_occurrence_ratio', 'aid_cart_last_week_occurrence_ratio', 'aid_order_last_week_occurrence_ratio',
    'aid_click_last_week_occurrence_pct_change', 'aid_cart_last_week_occurrence_pct_change',
    'aid_order_last_week_occurrence_pct_change',
    'aid_count', 'aid_session_nunique_rank_pct', 'aid_last_week_session_nunique')
SESSION_COLUMNS = (
    'session_count', 'session_aid_nunique', 'session_aid_last', 'session_type_last', 'session_day_of_week_last',
    'session_aid_count_mean', 'session_aid_count_min', 'session_aid_count_max', 'session_aid_count_last',
    'session_aid_type_mean_mean', 'session_aid_hour_mean_mean', 'session_aid_session_nunique_rank_pct_mean',
    'session_aid_session_nunique_rank_pct_last', 'session_aid_last_week_session_nunique_mean',
    'session_aid_last_week_session_nunique_last')
# integer rank sources, in the order of the device's rank keys
RANKED = ('count', 'days', 'tcount0', 'tcount1', 'tcount2', 'tsess0', 'tsess1', 'tsess2', 'tdays0', 'tdays1', 'tdays2',
          'lw_count', 'sess')
RANK_COLUMN = {'count': 8, 'days': 9, 'tcount0': 10, 'tcount1': 11, 'tcount2': 12, 'tsess0': 13, 'tsess1': 14, 'tsess2': 15,
               'tdays0': 16, 'tdays1': 17, 'tdays2': 18, 'lw_count': 19, 'sess': 29}
SRC_SCORE, SRC_INTER_ROW, SRC_INTER_SESSION, SRC_INTER_AID, SRC_AID, SRC_SESSION = range(6)
_EPOCH = datetime.date(1970, 1, 1).toordinal()


def day_table(day_min, day_max):
    """int32 [day_max - day_min + 1, 3]: day_of_week (Monday 0), day_of_year, ISO week_of_year of every day number."""
    out = np.zeros((day_max - day_min + 1, 3), dtype=np.int32)
    for i, d in enumerate(range(day_min, day_max + 1)):
        date = datetime.date.fromordinal(_EPOCH + d)
        out[i] = (date.weekday(), date.timetuple().tm_yday, date.isocalendar()[1])
    return out


def calendar(ts):
    """day number, hour, day_of_week, week_of_year per event (ts in seconds, shifted by two hours as the reference does)."""
    t = np.asarray(ts, dtype=np.int64) + 7200
    day = t // 86400
    hour = (t % 86400) // 3600
    if len(day) == 0:
        return day, hour, day.copy(), day.copy()
    tab = day_table(int(day.min()), int(day.max()))
    return day, hour, tab[day - day.min(), 0].astype(np.int64), tab[day - day.min(), 2].astype(np.int64)


def week_slots(week):
    """The weeks present, in order of first appearance in the event stream."""
    seen = []
    for w in week.tolist():
        if w not in seen:
            seen.append(w)
    return seen


def _f32(x):
    return np.float32(x)


def _div(a, b):
    """float64 a / b with IEEE results for a zero divisor (Python raises)."""
    a, b = float(a), float(b)
    if b == 0.0:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a)
    return a / b


def _mean_std(values):
    """(float32 mean, float32 sample std) of Python integers: exact integer sums, one division (and one sqrt)."""
    n, s, q = len(values), sum(values), sum(v * v for v in values)
    mean = _f32(s / n)
    std = _f32(math.sqrt((n * q - s * s) / (n * (n - 1)))) if n > 1 else _f32(np.nan)
    return mean, std


def rank_pct(values):
    """pandas ``rank(pct=True)`` (average method) of a list of integers with None for null: float32, NaN for null."""
    present = sorted(v for v in values if v is not None)
    arr = np.asarray(present, dtype=np.int64)
    out = np.full(len(values), np.nan, dtype=np.float32)
    for i, v in enumerate(values):
        if v is None:
            continue
        less = int(np.searchsorted(arr, v, side='left'))
        equal = int(np.searchsorted(arr, v, side='right')) - less
        out[i] = _f32((less + (equal + 1) / 2) / len(present))
    return out


def aid_table(aid, ts, typ, sess_off, n_aids):
    aid, ts, typ = np.asarray(aid, dtype=np.int64), np.asarray(ts, dtype=np.int64), np.asarray(typ, dtype=np.int64)
    sess_off = np.asarray(sess_off, dtype=np.int64)
    n = len(aid)
    out = np.full((n_aids, len(AID_COLUMNS)), np.nan, dtype=np.float32)
    if n == 0:
        return out
    day, hour, dow, week = calendar(ts)
    lens = np.diff(sess_off)
    sess = np.repeat(np.arange(len(lens)), lens)
    start = np.zeros(n, dtype=np.int64)
    end = np.zeros(n, dtype=np.int64)
    start[sess_off[:-1][lens > 0]] = 1
    end[sess_off[1:][lens > 0] - 1] = 1
    slots = week_slots(week)
    last_week = max(slots)
    by_aid = {}
    for i in range(n):
        by_aid.setdefault(int(aid[i]), []).append(i)
    ranked = {k: [None] * n_aids for k in RANKED}
    for a, ev in by_aid.items():
        ev = np.asarray(ev)
        m = len(ev)
        o = out[a]
        o[0] = _f32(int(typ[ev].sum()) / m)
        o[1], o[2] = _mean_std(hour[ev].tolist())
        o[3], o[4] = _mean_std(dow[ev].tolist())
        o[5] = _f32(_div(ts[ev].max(), ts[ev].min()))
        o[6] = _f32(int(start[ev].sum()) / m)
        o[7] = _f32(int(end[ev].sum()) / m)
        ranked['count'][a] = m
        ranked['days'][a] = len(set(day[ev].tolist()))
        ranked['sess'][a] = len(set(sess[ev].tolist()))
        for t in range(3):
            et = ev[typ[ev] == t]
            if len(et):
                ranked[f'tcount{t}'][a] = len(et)
                ranked[f'tsess{t}'][a] = len(set(sess[et].tolist()))
                ranked[f'tdays{t}'][a] = len(set(day[et].tolist()))
        lw = ev[week[ev] == last_week]
        if len(lw):
            ranked['lw_count'][a] = len(lw)
            o[20] = _f32(_div(ts[lw].max(), ts[lw].min()))
            o[21] = _f32(int(dow[lw].sum()) / len(lw))
            o[30] = _f32(len(set(sess[lw].tolist())))
        for t in range(3):
            c = [int(((week[ev] == w) & (typ[ev] == t)).sum()) for w in slots]
            r = _div(c[-1], sum(c))
            o[22 + t] = _f32(0.0 if r != r else r)
            pct = math.nan                                    # the last non-NaN change; +-inf counts and then becomes NaN
            for i in range(1, len(c)):
                p = _div(c[i], c[i - 1]) - 1.0
                if p == p:
                    pct = p
            o[25 + t] = _f32(math.nan if math.isinf(pct) else pct)
        o[28] = _f32(m)
    for k in RANKED:
        out[:, RANK_COLUMN[k]] = rank_pct(ranked[k])
    return out


def session_table(aid, ts, typ, sess_off, table):
    aid, typ = np.asarray(aid, dtype=np.int64), np.asarray(typ, dtype=np.int64)
    sess_off = np.asarray(sess_off, dtype=np.int64)
    S = len(sess_off) - 1
    out = np.full((S, len(SESSION_COLUMNS)), np.nan, dtype=np.float32)
    _, _, dow, _ = calendar(ts)

    def mean_last(col, ev):
        acc, cnt, last = 0.0, 0, np.float32(np.nan)
        for i in ev:
            v = table[aid[i], col]
            if v == v:
                acc += float(v)                                # float64, in event order
                cnt += 1
                last = v
        return (_f32(acc / cnt) if cnt else _f32(np.nan)), last

    for s in range(S):
        ev = range(int(sess_off[s]), int(sess_off[s + 1]))
        o = out[s]
        o[0] = len(ev)
        o[1] = len(set(aid[ev.start:ev.stop].tolist())) & 255
        if not len(ev):
            continue
        o[2], o[3], o[4] = aid[ev[-1]], typ[ev[-1]], dow[ev[-1]]
        cnt = [table[aid[i], 28] for i in ev]
        cnt = [v for v in cnt if v == v]
        o[5], o[8] = mean_last(28, ev)
        if cnt:
            o[6], o[7] = min(cnt), max(cnt)
        o[9], _ = mean_last(0, ev)
        o[10], _ = mean_last(1, ev)
        o[11], o[12] = mean_last(29, ev)
        o[13], o[14] = mean_last(30, ev)
    return out


def resolve(feature_names, inter_row_columns, inter_session_columns, inter_aid_columns):
    """(source, column) per name; ValueError listing the unknown names."""
    where = {'candidate_scores': (SRC_SCORE, 0)}
    for src, cols in ((SRC_INTER_ROW, inter_row_columns), (SRC_INTER_SESSION, inter_session_columns),
                      (SRC_INTER_AID, inter_aid_columns), (SRC_AID, AID_COLUMNS), (SRC_SESSION, SESSION_COLUMNS)):
        for q, name in enumerate(cols):
            where[name] = (src, q)
    unknown = [name for name in feature_names if name not in where]
    if unknown:
        raise ValueError(f'unknown feature names: {unknown}')
    return [where[name] for name in feature_names]


def matrix(row_off, cand, score, inter_row, inter_sess, inter_aid, aid_tab, sess_tab, program):
    """The float32 [n_rows, F] matrix by NumPy gathers. inter_row uint16 [n_rows, 5]."""
    row_off = np.asarray(row_off, dtype=np.int64)
    sess = np.repeat(np.arange(len(row_off) - 1), np.diff(row_off))
    n_rows = len(cand)
    out = np.empty((n_rows, len(program)), dtype=np.float32)
    for f, (src, col) in enumerate(program):
        if src == SRC_SCORE:
            out[:, f] = score
        elif src == SRC_INTER_ROW:
            v = inter_row[:, col].astype(np.float32)
            if col == 1:
                v[v == 0] = np.nan
            out[:, f] = v
        elif src == SRC_INTER_SESSION:
            out[:, f] = inter_sess[sess, col]
        elif src == SRC_INTER_AID:
            out[:, f] = inter_aid[cand, col]
        elif src == SRC_AID:
            out[:, f] = aid_tab[cand, col]
        else:
            out[:, f] = sess_tab[sess, col]
    return out
