"""Cut ``forest_order_fold1_head.lgb.txt``: the header and the first N trees of a LightGBM v3 text dump, ``tree_sizes``
trimmed to match, closed by ``end of trees``. Model weights only; no test runs this.

    python tests/golden/make_forest_head.py path/to/model_order_fold1.lgb [n_trees=8] > tests/golden/forest_order_fold1_head.lgb.txt
"""
import sys


def main():
    path = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    out = []
    with open(path) as f:
        for line in f:
            line = line.rstrip('\n')
            if line == f'Tree={n}' or line == 'end of trees':
                break
            if line.startswith('tree_sizes='):
                line = 'tree_sizes=' + ' '.join(line.split('=', 1)[1].split()[:n])
            out.append(line)
    while out and not out[-1]:
        out.pop()
    sys.stdout.write('\n'.join(out) + '\n\nend of trees\n')


if __name__ == '__main__':
    main()
