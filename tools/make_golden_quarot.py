"""Record the settings of the reference's QuaRot configurations for tests/test_quarot_config.py, so that the test runs from the
repository alone: every configs/quantization/**/*.yml whose `quant.method` is Quarot (step 1 of the QuaRot + GPTQ pipelines,
methods/QuaRot/*) and the `step_2_gptq.yml` lying next to a `step_1_quarot.yml` (GPTQ with online_rotate). Settings only.

    python tools/make_golden_quarot.py <path of the reference tree>        -> tests/golden/ref_quarot_configs.json
(or LLMC_REFERENCE in the environment)"""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def collect(ref):
    import yaml
    base = os.path.join(ref, 'configs', 'quantization')
    out = {}
    for f in sorted(glob.glob(base + '/**/*.yml', recursive=True)):
        try:
            c = yaml.safe_load(open(f))
        except Exception:       # noqa: BLE001
            continue
        q = (c or {}).get('quant') or {}
        if not isinstance(q, dict):
            continue
        step2 = os.path.basename(f) == 'step_2_gptq.yml' and os.path.exists(os.path.join(os.path.dirname(f), 'step_1_quarot.yml'))
        if q.get('method') == 'Quarot' or step2:
            assert json.loads(json.dumps(c)) == c, f
            out[os.path.relpath(f, base)] = c
    return out


if __name__ == '__main__':
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('LLMC_REFERENCE')
    if not ref:
        sys.exit(__doc__)
    cfgs = collect(ref)
    path = os.path.join(ROOT, 'tests', 'golden', 'ref_quarot_configs.json')
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
    print(f'{len(cfgs)} configurations -> {path}')
