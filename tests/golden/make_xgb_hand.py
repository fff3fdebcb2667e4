"""Writes tests/golden/xgb_hand.json: two SPEC-XGB cases small enough to follow on paper. Nothing here calls the
restatement or the package: the draws, the pairs and the splits are written out below, and the expected numbers are the
arithmetic of the spec typed in, operation by operation. tests/test_xgb_cpu.py holds the restatement to this file.

Case 1: rank:pairwise on one query of 5 rows, xgb seed 7 (objective_seed = mix(7, 1) = 309689372594955804), iteration 0
(seed_it = mix(objective_seed, 0) = 9391409690812996836).

    row    0     1     2     3     4
    score  0.5   0.5  -1.0   2.0   0.0
    label  1     0     2     1     0

  Rank (score descending, position ascending): rows 3, 0, 1, 4, 2 -- rows 0 and 1 tie at 0.5 and keep their positions.
  Labels by rank: 1, 1, 0, 0, 2.
  Record order (label descending, rank ascending): ranks 4, 0, 1, 2, 3 = rows 2, 3, 0, 1, 4.
  Buckets of rec: label 2 = [0, 1): nleft 0, nright 4, m 4;  label 1 = [1, 3): nleft 1, nright 2, m 3;
                  label 0 = [3, 5): nleft 3, nright 0, m 3.
  Draws, u = mix(seed_it, row) mod m:
    pid 0  row 2  mix = 348166758678467524    mod 4 = 0   u >= nleft: high = row 2, low = rec[0 + 1] = row 3
    pid 1  row 3  mix = 7809585962377632801   mod 3 = 0   u <  nleft: high = rec[0] = row 2, low = row 3
    pid 2  row 0  mix = 16752092399367933723  mod 3 = 0   u <  nleft: high = rec[0] = row 2, low = row 0
    pid 3  row 1  mix = 13005527499740442230  mod 3 = 2   u <  nleft: high = rec[2] = row 0, low = row 1
    pid 4  row 4  mix = 1280629128021953582   mod 3 = 2   u <  nleft: high = rec[2] = row 0, low = row 4
  Pair terms, d = s_low - s_high, p = T[(d + 25) * 20971.52] = 1 / (1 + exp(-25 + index / 20971.52)):
    pid 0, 1  d =  3.0  index 587202  p = 0.04742707953910805
    pid 2     d =  1.5  index 555745  p = 0.18242751513476982
    pid 3     d =  0.0  index 524288  p = 0.5
    pid 4     d = -0.5  index 513802  p = 0.6224620206021405
  Sums, every row in ascending pid:
    row 2: high in pids 0, 1, 2        row 3: low in pids 0, 1        row 0: low in pid 2, high in pids 3, 4
    row 1: low in pid 3                row 4: low in pid 4

Case 2: one depth-2 tree over 12 rows, 2 features, e_g = e_h = 0 (so G = sum qg, H = sum qh), qh = 1 everywhere,
lambda 1, min_child_weight 1, gamma 0, eta 0.5.

    row      0   1   2   3   4   5   6   7   8   9  10  11
    bin f0   0   0   0   1   1   1   2   2   2   3   3   3      edges 1.0, 2.0, 3.0
    bin f1   0   1   0   1   0   1   0   1   0   1   0   1      edge 0.5
    qg      -4  -3  -4  -1  -2  -1   2   3   2   5   4   5

  Root (id 0): G = 6, H = 12. f0: b0 121/4 + 289/10 - 36/13; b1 225/7 + 441/7 - 36/13 (the best); b2 64/10 + 196/4 - 36/13.
    f1 b0: 4/7 + 64/7 - 36/13. No NaN row: both NaN variants tie, NaN-right wins. Left = rows 0..5 (id 1), right = 6..11 (id 2).
  Level 1, id 1 (G = -15, H = 6): f0 b0 121/4 + 16/4 - 225/7 > 0 (the best); f0 b1 leaves no row right (H_R = 0 < 1);
    f1 b0 100/4 + 25/4 - 225/7 < 0. Splits into ids 3 (rows 0..2) and 4 (rows 3..5).
  Level 1, id 2 (G = 21, H = 6): f0 b2 49/4 + 196/4 - 441/7 < 0; f1 b0 64/4 + 169/4 - 63 < 0; f0 b0, b1 leave no row left.
    No split: id 2 stays a leaf while its sibling splits -- the level has a gap.
  BinTree: node 0 = (f0, b1), left -> node 1, right -> leaf 1; node 1 = (f0, b0), left -> leaf 0, right -> leaf 2.
  Leaves: leaf 0 = rows 0..2 (G -11, H 3), leaf 1 = rows 6..11 (G 21, H 6), leaf 2 = rows 3..5 (G -4, H 3).
  Histograms read: the root (12 rows), then the smaller child of the root's split (6 : 6, a tie: the left one, 6 rows).
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    p01, p2, p3, p4 = 0.04742707953910805, 0.18242751513476982, 0.5, 0.6224620206021405
    g01, g2, g3, g4 = p01 - 1.0, p2 - 1.0, p3 - 1.0, p4 - 1.0
    h01, h2, h3, h4 = 2.0 * (p01 * (1.0 - p01)), 2.0 * (p2 * (1.0 - p2)), 2.0 * (p3 * (1.0 - p3)), 2.0 * (p4 * (1.0 - p4))
    grad = [((0.0 - g2) + g3) + g4, 0.0 - g3, ((0.0 + g01) + g01) + g2, (0.0 - g01) - g01, 0.0 - g4]
    hess = [((0.0 + h2) + h3) + h4, 0.0 + h3, ((0.0 + h01) + h01) + h2, (0.0 + h01) + h01, 0.0 + h4]
    objective = dict(seed=7, it=0, score=[0.5, 0.5, -1.0, 2.0, 0.0], label=[1, 0, 2, 1, 0], query_off=[0, 5],
                     rec_rows=[2, 3, 0, 1, 4], pairs_rows=[[2, 3], [2, 3], [2, 0], [0, 1], [0, 4]], grad=grad, hess=hess)
    eta = 0.5
    tree = dict(
        bins=[[0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3], [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1]],
        edges=[[1.0, 2.0, 3.0], [0.5]],
        qg=[-4, -3, -4, -1, -2, -1, 2, 3, 2, 5, 4, 5], qh=[1] * 12, exps=[0, 0],
        params={'max_depth': 2, 'lambda': 1.0, 'min_child_weight': 1.0, 'gamma': 0.0, 'eta': eta},
        split_feature=[0, 0], split_bin=[1, 0], default_left=[0, 0], threshold=[2.0, 1.0], left_child=[1, -1], right_child=[-2, -3],
        split_gain=[(225.0 / 7.0 + 441.0 / 7.0) - 36.0 / 13.0, (121.0 / 4.0 + 16.0 / 4.0) - 225.0 / 7.0],
        cover=[12.0, 6.0], sum_grad=[6.0, -15.0], count=[12, 6], left_id=[1, 3], right_id=[2, 4],
        leaf_value=[-(-11.0 / 4.0) * eta, -(21.0 / 7.0) * eta, -(-4.0 / 4.0) * eta], leaf_cover=[3.0, 6.0, 3.0],
        leaf_sum_grad=[-11.0, 21.0, -4.0], leaf_count=[3, 6, 3], hist_rows=18)
    with open(os.path.join(HERE, 'xgb_hand.json'), 'w') as f:
        json.dump(dict(objective=objective, tree=tree), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
