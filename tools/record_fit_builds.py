""" Record which builds of the fused kernel the library launches over the decision space of tests/test_gpu_build_sweep.py (needs a GPU).

    python tools/record_fit_builds.py --commit HASH [--out tests/golden/fit_build_choices.json]

Runs tests/_fit_build_choices.py on the tree this file lies in and writes {"commit": HASH, "choices": {configuration: {case: {record:
launches}}}} -- `commit` names the commit whose build made the record.  tests/test_gpu_fit_build_choices.py holds every later tree to
it; a change of launch policy re-records the file on purpose, and the diff of the JSON shows which shape moved to which build.
(Records in short spelling: apply<MODEL,R2,RW,DENSE,RING,CERT_ONLY,WPB,BATCH> = fit_apply_kernel<...>, list<MODEL,R2,RW,DENSE,RING> =
fit_list_kernel<...>.) """
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def write(record, path):
    """ one case per line, so that a re-recording shows as one changed line per case that moved """
    with open(path, 'w') as f:
        f.write('{"commit": %s, "choices": {\n' % json.dumps(record['commit']))
        for i, (config, cases) in enumerate(record['choices'].items()):
            f.write('%s: {\n' % json.dumps(config))
            f.write(',\n'.join('  %s: %s' % (json.dumps(case), json.dumps(hits, separators=(',', ':'))) for case, hits in cases.items()))
            f.write('\n}%s\n' % (',' if i + 1 < len(record['choices']) else ''))
        f.write('}}\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit this tree is a checkout of')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden', 'fit_build_choices.json'))
    args = ap.parse_args()
    import _fit_build_choices as fbc
    record = {'commit': args.commit, 'choices': {}}
    for config in fbc.CONFIGS:
        record['choices'][fbc.config_id(*config)] = fbc.choices(config)
        print(fbc.config_id(*config), len(record['choices'][fbc.config_id(*config)]), 'cases', flush=True)
    write(record, args.out)
