"""Writes tests/golden/objectives_hand.json: SPEC-OBJ cases small enough to follow on paper. Nothing here calls the
restatement or the package: exact values are worked with ``fractions``, the ones that hold a logarithm with ``decimal`` at 50
digits and rounded once to float64. tests/test_objectives_cpu.py holds the restatement to this file (exact values bit for
bit, the rounded ones to 4 ulp: the spec rounds after every operation, the fixture once).

binary.  A score of 0.0 reads the table's middle entry, index (0 + 25) * 2^20 / 50 = 524288 exactly, p = 1 / (1 + exp(0)) =
  1/2. sigma = 2, w_pos = 3, w_neg = 1, floor 0:
    label 1: grad = 2 * (1/2 - 1) * 3 = -3      hess = 2 * 2 * 1/2 * 1/2 * 3 = 3
    label 0: grad = 2 * (1/2 - 0) * 1 =  1      hess = 2 * 2 * 1/2 * 1/2 * 1 = 1
weights. 3 positives among 12 rows, is_unbalance: the negatives are the larger class: w_neg = 1, w_pos = 9 / 3 = 3.
    12 positives among 16 rows: w_pos = 1, w_neg = 12 / 4 = 3. scale_pos_weight 2.5 without is_unbalance: (2.5, 1).
init.    1 positive among 4 rows, sigma 2: pavg = 1/4, init = ln((1/4) / (3/4)) / 2 = -ln(3) / 2.
         no positive among 4 rows, sigma 1: pavg = 1e-15, init = ln(1e-15 / (1 - 1e-15)).
margin.  base_score 1/2 -> 0 exactly; base_score 1/5 -> ln(1/4) = -2 ln 2.
auc.     score 0.9 0.8 0.8 0.7 0.7 0.1, label 1 1 0 0 1 0: P = 3, N = 3. Over all 9 (positive, negative) pairs:
    the positive at 0.9 beats 3 negatives; the one at 0.8 ties one, beats two: 2.5; the one at 0.7 loses one, ties one, beats
    one: 1.5. Sum 7, A2 = 14, AUC = 7/9. By tie groups of the descending order [0.9] [0.8 0.8] [0.7 0.7] [0.1] with
    Ppre = 0 1 2 2 2 3 3: 0*(0+1) + 1*(1+2) + 1*(2+3) + 1*(3+3) = 14.
ndcg.    One query in rank order with labels 2 0 1 3 (gains 3 0 1 7), discounts 1, 1/log2(3), 1/2, 1/log2(5):
    k = 1: DCG = 3, maxDCG = 7: 3/7.   k = 4: DCG = 3 + 1/2 + 7/log2(5), maxDCG = 7 + 3/log2(3) + 1/2.
logloss. Three rows at score 0: 3 * ln 2, whatever the labels. One positive at sigma * score = 800: ln(1 + exp(-800)),
    below 1e-347: 0.0 in float64; one negative there: 800 + the same = 800.
lambdamart. One query of two rows, scores 0 0, labels 2 0. Rank = position. IDCG = 3 * 1: inv_idcg = 1/3. Both rows draw
    the other one (m = 1), so the pair (high = row 0, low = row 1) is there twice, at pid 0 and pid 1. d = 0: p = 1/2.
    delta = |(3 - 0) * (1 - 1/log2(3))| / 3 = 1 - 1/log2(3); g = -delta/2; h2 = 2 * 1/4 * delta = delta/2.
    grad = (-delta, +delta), hess = (delta, delta).
"""
import json
import os
from decimal import Decimal, getcontext
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
getcontext().prec = 50


def log2(x):
    return Decimal(x).ln() / Decimal(2).ln()


def main():
    ln2, ln3 = Decimal(2).ln(), Decimal(3).ln()
    tiny = Decimal('1e-15')
    # float(1 - 1e-15) is not 1 - 1e-15: the spec clips to the float64 bounds, so the fixture works from those
    lo = Decimal(float(tiny))
    delta = 1 - 1 / log2(3)
    hand = {
        'binary': {'score': [0.0, 0.0], 'label': [1, 0], 'sigma': 2.0, 'w_pos': 3.0, 'w_neg': 1.0, 'hess_floor': 0.0,
                   'grad': [float(Fraction(2) * (Fraction(1, 2) - 1) * 3), float(Fraction(2) * Fraction(1, 2) * 1)],
                   'hess': [float(Fraction(4) * Fraction(1, 4) * 3), float(Fraction(4) * Fraction(1, 4) * 1)]},
        'weights': [{'n_pos': 3, 'n': 12, 'is_unbalance': True, 'scale_pos_weight': 1.0, 'w': [float(Fraction(9, 3)), 1.0]},
                    {'n_pos': 12, 'n': 16, 'is_unbalance': True, 'scale_pos_weight': 1.0, 'w': [1.0, float(Fraction(12, 4))]},
                    {'n_pos': 3, 'n': 12, 'is_unbalance': False, 'scale_pos_weight': 2.5, 'w': [2.5, 1.0]}],
        'init': [{'n_pos': 1, 'n': 4, 'sigma': 2.0, 'value': float(-ln3 / 2)},
                 {'n_pos': 0, 'n': 4, 'sigma': 1.0, 'value': float((lo / (1 - lo)).ln())}],
        'margin': [{'base_score': 0.5, 'value': 0.0}, {'base_score': 0.2, 'value': float((Decimal(0.2) / (1 - Decimal(0.2))).ln())}],
        'auc': {'score': [0.9, 0.8, 0.8, 0.7, 0.7, 0.1], 'label': [1, 1, 0, 0, 1, 0], 'a2': 14, 'p': 3, 'n': 3,
                'auc': float(Fraction(14, 2 * 3 * 3))},
        'ndcg': {'score': [4.0, 3.0, 2.0, 1.0], 'label': [2, 0, 1, 3],
                 'at_1': float(Fraction(3, 7)),
                 'at_4': float((3 + Decimal(1) / 2 + 7 / log2(5)) / (7 + 3 / log2(3) + Decimal(1) / 2))},
        'logloss': {'zeros': float(3 * ln2), 'positive_at_800': 0.0, 'negative_at_800': 800.0},
        'lambdamart': {'score': [0.0, 0.0], 'label': [2, 0], 'grad': [float(-delta), float(delta)], 'hess': [float(delta), float(delta)]},
    }
    with open(os.path.join(HERE, 'objectives_hand.json'), 'w') as f:
        json.dump(hand, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
