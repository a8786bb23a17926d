"""Every YAML the reference ships under configs/quantization/ for the four registered algorithms (GPTQ, Awq, RTN, SpQR), read as it
is: the mirrored class either accepts the `quant` section at construction (config plumbing, quantizer construction, special keys —
no compute) or refuses it with a NotImplementedError that says why. The files are read from tests/golden/ref_quant_configs.json
(recorded from the reference by oracle/make_golden_configs.py); the table it produces is committed as
profiles/r04_config_acceptance.txt."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_quant_configs.json')

ALGOS = ('GPTQ', 'Awq', 'RTN', 'SpQR')
# configurations of the four algorithms that leave the path: what the refusal must mention
EXPECTED_REFUSALS = {
    'kvcache': 'KV-cache',                 # quant.kvcache
    'bit48': 'W48',                        # weight.bit: 48 (int4 weights with int8 second-level scales)
    'quant_attn': 'attention',             # act.quant_attn / quant_act_fn
    'hqq': 'hqq',                          # calib_algo: hqq
    'modality': 'modalit',                 # vision / audio towers (quant.vision, quant.audio ...)
}


def shipped():
    with open(GOLDEN) as f:
        configs = json.load(f)
    out = []
    for rel in sorted(configs):
        c = configs[rel]
        q = (c or {}).get('quant') or {}
        if isinstance(q, dict) and q.get('method') in ALGOS:
            out.append((rel, c))
    return out


def construct(cfg):
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    model = ToyModel()
    q = dict(cfg['quant'])
    sp = dict(q.get('special') or {})
    for k in ('scale_path', 'clip_path'):          # placeholders of the shipped files
        if k in sp:
            sp[k] = '/tmp/llmc_amd_cfg_' + k
    if sp:
        q['special'] = sp
    config = {'calib': cfg.get('calib') or {}, 'model': cfg.get('model') or {}, 'quant': q}
    if 'ignored_layers' in cfg:
        config['ignored_layers'] = cfg['ignored_layers']
    cls = getattr(Q, q['method'])
    if hasattr(cls, 'collect_model_qparams'):
        # GPTQ.__init__ evaluates the static min/max qparams of every block on the GPU, like the reference's (gptq.py:31,
        # 325-333): compute, not configuration — skipped here (the GPU suite constructs the class for real)
        class NoCollect(cls):
            def collect_model_qparams(self):
                pass
        cls = NoCollect
    return cls(model, q, calib_input(model), None, config)


def test_every_shipped_configuration_is_accepted_or_refused_with_a_reason():
    rows, bad = [], []
    files = shipped()
    assert len(files) >= 60
    for rel, cfg in files:
        q = cfg['quant']
        try:
            construct(cfg)
            rows.append((rel, q['method'], 'accepted', ''))
        except NotImplementedError as e:
            rows.append((rel, q['method'], 'refused', str(e).split('\n')[0][:110]))
        except Exception as e:      # noqa: BLE001
            rows.append((rel, q['method'], 'ERROR', f'{type(e).__name__}: {e}'[:110]))
            bad.append(rel)
    out = os.environ.get('LLMC_CONFIG_TABLE')
    if out:
        with open(out, 'w') as f:
            f.write('# configs/quantization/**/*.yml of the reference with method GPTQ / Awq / RTN / SpQR, constructed with llmc_amd '
                    '(tests/test_config_acceptance.py)\n')
            acc = sum(r[2] == 'accepted' for r in rows)
            f.write(f'# {len(rows)} files: {acc} accepted, {sum(r[2] == "refused" for r in rows)} refused with a reason, '
                    f'{len(bad)} errors\n')
            for r in rows:
                f.write(f'{r[2]:9s} {r[1]:5s} {r[0]:78s} {r[3]}\n')
    assert not bad, bad
    accepted = [r for r in rows if r[2] == 'accepted']
    assert len(accepted) >= 0.75 * len(rows), (len(accepted), len(rows))
    for r in rows:
        if r[2] == 'refused':
            assert r[3], r          # a refusal always says what it refuses
