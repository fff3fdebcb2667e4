"""Writes tests/golden/gbdt_sampling_hand.json: the sampler of SPEC-GBDT worked with scalar Python integers alone. It shares
no code with tests/gbdt_sampling_restatement.py or the package: the formula is typed out again from the header.

    python tests/golden/make_gbdt_sampling_hand.py
"""
import json
import os

MASK = 0xFFFFFFFFFFFFFFFF


def mix(s, i):
    z = (s + (i + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def smallest(keys, count):
    order = sorted(range(len(keys)), key=lambda i: keys[i])
    return sorted(order[:count])


def compute():
    n, p, bagging_seed = 16, 0.5, 42
    m = int(p * n)
    bags = []
    for d in (0, 1):
        seed = mix(bagging_seed, 2 * d)
        bags.append({'draw': d, 'seed': str(seed), 'rows': smallest([mix(seed, r) for r in range(n)], m)})
    F, q, feature_seed = 10, 0.5, 42
    n_used = max(min(2, F), int(F * q + 0.5))
    lists = []
    for it in (0, 1):
        seed = mix(feature_seed, 2 * it + 1)
        lists.append({'iteration': it, 'features': smallest([mix(seed, f) for f in range(F)], n_used)})
    points = [(0, 0), (0, 1), (42, 0), (42, 7), (3, 2 ** 31 - 1), (MASK, 0), (MASK, 1), (MASK, MASK)]
    return {'mix': [{'s': str(s), 'i': str(i), 'value': str(mix(s, i))} for s, i in points],
            'bag': {'n': n, 'bagging_fraction': p, 'bagging_seed': bagging_seed, 'm': m, 'draws': bags},
            'features': {'F': F, 'feature_fraction': q, 'feature_fraction_seed': feature_seed, 'n_used': n_used, 'iterations': lists}}


if __name__ == '__main__':
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'gbdt_sampling_hand.json'), 'w') as fh:
        json.dump(compute(), fh, indent=1)
        fh.write('\n')
