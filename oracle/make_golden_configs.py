"""Record the reference data that three CPU tests compare against, so that they run from the repository alone:

  tests/golden/ref_quant_configs.json   every configs/quantization/**/*.yml of the reference whose `quant.method` is GPTQ,
                                        Awq, RTN or SpQR, parsed (settings only): tests/test_config_acceptance.py
  tests/golden/export_config.json       what the reference's own exporters (llmc/utils/export_vllm.py, export_autoawq.py)
                                        write into config.json for the cases of tests/test_export_config.py

Run where the reference tree exists (LLMC_REFERENCE, default as in oracle/build_ref.py):
    python oracle/make_golden_configs.py
Test infrastructure only."""
import glob
import importlib.util
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, HERE)
from build_ref import REF  # noqa: E402

ALGOS = ('GPTQ', 'Awq', 'RTN', 'SpQR')


def quant_configs():
    import yaml
    base = os.path.join(REF, 'configs', 'quantization')
    out = {}
    for f in sorted(glob.glob(base + '/**/*.yml', recursive=True)):
        try:
            c = yaml.safe_load(open(f))
        except Exception:       # noqa: BLE001
            continue
        q = (c or {}).get('quant') or {}
        if isinstance(q, dict) and q.get('method') in ALGOS:
            rel = os.path.relpath(f, base)
            assert json.loads(json.dumps(c)) == c, f'{rel} does not survive JSON'
            out[rel] = c
    return out


def _load_ref(name):
    spec = importlib.util.spec_from_file_location('ref_' + name, os.path.join(REF, 'llmc', 'utils', name + '.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def export_configs():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_export_config as T
    vllm, awq = _load_ref('export_vllm'), _load_ref('export_autoawq')
    out = {'vllm': {}, 'autoawq': []}
    with tempfile.TemporaryDirectory() as tmp:
        for case in sorted(T.CASES):
            d = os.path.join(tmp, 'vllm_' + case)
            out['vllm'][case] = T._run(vllm.update_vllm_quant_config, d, T.Model(), T.cfg({'quant': T.CASES[case]}), d)
        for i, w in enumerate(T.AUTOAWQ_CASES):
            d = os.path.join(tmp, f'autoawq_{i}')
            out['autoawq'].append(T._run(awq.update_autoawq_quant_config, d, T.cfg({'quant': {'weight': w}}), d))
    return out


def write(name, obj):
    path = os.path.join(GOLD, name)
    with open(path, 'w') as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)')


if __name__ == '__main__':
    if not os.path.isdir(os.path.join(REF, 'llmc')):
        raise SystemExit(f'reference tree not found at {REF} (set LLMC_REFERENCE)')
    write('ref_quant_configs.json', quant_configs())
    write('export_config.json', export_configs())
