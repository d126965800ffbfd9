"""The DeepEMD head over a labelled support set: fsvit_emd_bank_accumulate / fsvit_emd_bank_finalize / fsvit_emd_rerank behind ops.emd_bank_* and
ops.emd_rerank, models.emd_bank.TokenBank, DeepEMD.fit / predict / predict_topk and `python -m fewshot_vit_amd.predict --head deepemd`.

References: the sums against float64 with the rounding of an fp32 chain; what the bank promises bit for bit (a split fill, the node preparation, the
re-rank against the dense route, the module and the CLI against the calls they are made of) with `==`; the re-ranked logits against the float64
oracle of tests/emd_bank_cases.py by the 1e-4 that tests/test_gpu_emd.py derives for the head.  No order is compared with the float64 oracle (its
consecutive logits come as close as 4.9e-5): the order is checked exactly against the GPU's own dense logits, and against the oracle only up to
2e-4 of slack, which is safe under near-ties."""
import csv
import os

import numpy as np
import pytest
import torch

import emd_bank_cases as bc

pytestmark = pytest.mark.gpu
T = bc.T
TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8)       # the encoder of test_gpu_predict_cli.py
ENCODER = 'tiny_visformer_emd_bank'
CLASSES = ('ant', 'bee', 'cat')
SHOTS5 = (3, 0, 1, 4, 2)


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


def _state(n_classes, N, Cc):
    return (torch.zeros(n_classes, N, Cc, device='cuda'), torch.zeros(n_classes, dtype=torch.int32, device='cuda'),
            torch.zeros(1, dtype=torch.int32, device='cuda'))


# ---------------------------------------------------------------- 1. accumulate / finalize
@pytest.mark.parametrize('C', [64, 320])
@pytest.mark.parametrize('N', [1, 7, 25, 32])
def test_accumulate_and_finalize(N, C):
    """Sums: a class's s rows are added one by one on top of a stored zero, so s - 1 of the additions round, each by at most 2^-24 of a partial sum
    that is at most sum |x|: |sum - float64| <= (s - 1) * 2^-24 * sum |x| per element (zero for a 1-shot class: its sum is the row)."""
    ops = _ops()
    case = bc.bank_case(5, SHOTS5, 1, N, C, seed=N + C)
    sup, lab = case['sup'].float().cuda(), case['sup_lab'].cuda()
    one = _state(5, N, C)
    ops.emd_bank_accumulate(sup, lab, *one)
    assert one[1].tolist() == list(SHOTS5) and int(one[2]) == 0
    ref = torch.zeros(5, N, C, dtype=torch.float64)
    mag = torch.zeros(5, N, C, dtype=torch.float64)
    ref.index_add_(0, case['sup_lab'], case['sup'])
    mag.index_add_(0, case['sup_lab'], case['sup'].abs())
    bound = (torch.tensor(SHOTS5, dtype=torch.float64) - 1).clamp_min(0)[:, None, None] * 2.0 ** -24 * mag
    err = (one[0].cpu().double() - ref).abs()
    print(f'emd_bank_accumulate N={N} C={C}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}')
    assert bool((err <= bound).all())
    # a split fill, int32 labels on one side: the bits of one call
    two = _state(5, N, C)
    ops.emd_bank_accumulate(sup[:4], lab[:4].int(), *two)
    ops.emd_bank_accumulate(sup[4:], lab[4:], *two)
    ops.emd_bank_accumulate(sup[:0], lab[:0], *two)                                # S == 0: a no-op
    assert torch.equal(two[0], one[0]) and torch.equal(two[1], one[1]) and int(two[2]) == 0
    # two labels outside [0, 5): counted, and their (huge) rows reach no sum
    for dtype in (torch.int32, torch.int64):
        bad = _state(5, N, C)
        sup_b = torch.cat([sup[:3], torch.full((1, N, C), 1e30, device='cuda'), sup[3:], torch.full((1, N, C), -1e30, device='cuda')])
        lab_b = torch.cat([lab[:3], torch.tensor([5], device='cuda'), lab[3:], torch.tensor([-1], device='cuda')]).to(dtype)
        ops.emd_bank_accumulate(sup_b, lab_b, *bad)
        assert int(bad[2]) == 2 and torch.equal(bad[0], one[0]) and torch.equal(bad[1], one[1])
    # finalize
    tok, xhat, pooled, proto, empty = ops.emd_bank_finalize(one[0], one[1])
    assert empty.tolist() == [0, 1, 0, 0, 0]
    quot = one[0].cpu().double() / torch.tensor(SHOTS5, dtype=torch.float64).clamp_min(1)[:, None, None]
    assert bool(((tok.cpu().double() - quot).abs() <= 2.0 ** -23 * quot.abs()).all())      # one fp32 division: within a unit in the last place
    xh, pl = torch.full_like(tok, float('nan')), torch.full_like(pooled, float('nan'))
    ops.emd_table_prep(tok, xh, pl)
    filled = [0, 2, 3, 4]
    assert torch.equal(xhat[filled], xh[filled]) and torch.equal(pooled[filled], pl[filled])
    for t in (tok, xhat, pooled, proto):
        assert float(t[1].abs().max()) == 0.0                                     # the class without examples: zero rows
    ref_proto = torch.nn.functional.normalize(pooled.cpu().double(), dim=-1, eps=1e-12)
    assert (proto.cpu().double() - ref_proto).abs().max().item() <= 1e-6
    assert (proto[filled].double().norm(dim=-1) - 1).abs().max().item() <= 1e-6


# ---------------------------------------------------------------- 2. re-rank against the dense route (bitwise)
_banks = {}


def _bank(key):
    """key = the arguments of bank_case -> (case, TokenBank, query maps on the GPU, dense GPU logits [Q,n_classes]); built once, never modified"""
    if key not in _banks:
        from fewshot_vit_amd.models.emd_bank import TokenBank
        case = bc.bank_case(*key)
        bank = TokenBank(key[0], key[3], key[4], 'cuda').add(case['sup'].float().cuda(), case['sup_lab'].cuda())
        bank.check()
        qry = case['qry'].float().cuda()
        _banks[key] = (case, bank, qry, bank.logits(qry, T))
    return _banks[key]


def _rerank(bank, qry, cand, k, want_logits=False):
    ops = _ops()
    xhat, pooled = torch.empty_like(qry), torch.empty(qry.shape[0], qry.shape[2], device='cuda')
    ops.emd_table_prep(qry, xhat, pooled)
    m = bank.class_maps()
    return ops.emd_rerank((qry, xhat, pooled), (m[0], m[1], m[2], m[4]), cand.to(torch.int32).cuda(), T, k, want_logits=want_logits)


def _expect(dense, cand, n_classes):
    """(classes [Q,M], values [Q,M]) of the stated order over the dense logits restricted to cand (host tensors); a bad candidate is an empty slot"""
    classes, values = [], []
    for row, cs in zip(dense.cpu(), cand.tolist()):
        cs = [c if 0 <= c < n_classes else -1 for c in cs]
        vs = [float(row[c]) if c >= 0 else float('-inf') for c in cs]
        order = bc.ranked(vs, cs)
        classes.append([cs[i] for i in order])
        values.append([vs[i] for i in order])
    return torch.tensor(classes, dtype=torch.int32), torch.tensor(values, dtype=torch.float32)


@pytest.mark.parametrize('Q', [1, 5])
@pytest.mark.parametrize('N', [7, 25])
def test_rerank_equals_the_dense_route(N, Q):
    """M = 1, 5, 12 with 4 waves per query: one wave alone, uneven waves, three rounds."""
    case, bank, qry, dense = _bank((12, 3, Q, N, 64, N))
    assert bool(torch.isneginf(dense[:, 1]).all()) and bool(torch.isfinite(dense[:, [c for c in range(12) if c != 1]]).all())
    full = torch.arange(12).repeat(Q, 1)
    classes, values, prob, logits, status, invalid = _rerank(bank, qry, full, 12, want_logits=True)
    assert torch.equal(logits, dense), 'the re-rank does not give the bits of the dense route'
    assert int(status) == 0 and int(invalid) == 0
    g = torch.Generator().manual_seed(N * 10 + Q)
    for M in (1, 5, 12):
        cand = torch.stack([torch.randperm(12, generator=g)[:M] for _ in range(Q)])
        if M == 5:
            cand[0, 2] = 1                                                        # the class without examples among them
        ref_c, ref_v = _expect(dense, cand, 12)
        for k in sorted({1, M}):
            classes, values, prob, logits, status, invalid = _rerank(bank, qry, cand, k)
            assert logits is None and classes.dtype == torch.int32 and classes.shape == (Q, k)
            assert torch.equal(classes.cpu(), ref_c[:, :k]) and torch.equal(values.cpu(), ref_v[:, :k]), (M, k)
            assert int(status) == 0 and int(invalid) == 0
    assert int(bank.status_count) == 0


def test_rerank_of_32_candidates():
    case, bank, qry, dense = _bank((40, 3, 5, 7, 64, 3))
    g = torch.Generator().manual_seed(32)
    cand = torch.stack([torch.randperm(40, generator=g)[:32] for _ in range(5)])
    ref_c, ref_v = _expect(dense, cand, 40)
    classes, values, prob, logits, status, invalid = _rerank(bank, qry, cand, 32, want_logits=True)
    assert torch.equal(classes.cpu(), ref_c) and torch.equal(values.cpu(), ref_v)
    assert torch.equal(logits.cpu(), torch.gather(dense.cpu(), 1, cand)) and int(status) == 0 and int(invalid) == 0
    # the shortlist of TokenBank.topk: 32 classes by the cosine of token means, re-ranked - every returned logit is the dense one of its class
    top_c, top_v, top_p = bank.topk(qry, 5, T)
    assert top_c.dtype == torch.int64 and torch.equal(top_v, torch.gather(dense, 1, top_c))
    assert bool((top_v[:, :-1] >= top_v[:, 1:]).all()) and int(bank.status_count) == 0


def test_hand_made_candidate_rows():
    """-1, a duplicate, the class without examples and one entry outside the bank: the bad entry is counted and becomes an empty slot, never an address"""
    case, bank, qry, dense = _bank((12, 3, 5, 25, 64, 25))
    good = torch.tensor([[3, 4, 5, 6, 7], [2, 0, 8, 9, 5], [11, 10, 9, 8, 7], [0, 2, 3, 4, 5], [6, 5, 4, 3, 2]])
    cand = good.clone()
    cand[0] = torch.tensor([3, -1, 3, 1, 7])
    cand[1, 2] = 12                                                               # n_classes itself
    ref_c, ref_v = _expect(dense, cand, 12)
    classes, values, prob, logits, status, invalid = _rerank(bank, qry, cand, 5, want_logits=True)
    assert int(invalid) == 1 and int(status) == 0
    assert torch.equal(classes.cpu(), ref_c) and torch.equal(values.cpu(), ref_v)
    # the duplicate is scored twice; at the end the class without examples, then the empty slot
    assert sorted(classes[0].tolist()[:3]) == [3, 3, 7] and classes[0].tolist()[3:] == [1, -1] and bool(torch.isneginf(values[0, 3:]).all())
    assert classes[1, 4].item() == -1 and torch.isneginf(values[1, 4]).item() and torch.isneginf(logits[1, 2]).item()
    assert prob[0, 3:].tolist() == [0.0, 0.0] and prob[1, 4].item() == 0.0 and abs(prob[0].sum().item() - 1) <= 1e-5
    clean = _rerank(bank, qry, good, 5)
    assert torch.equal(classes[2:], clean[0][2:]) and torch.equal(values[2:], clean[1][2:]) and torch.equal(prob[2:], clean[2][2:])
    # TokenBank.topk with the caller's candidates, int64: an entry beyond int32 is out of range, not the class it would wrap to
    from fewshot_vit_amd.models.emd_bank import TokenBank
    own = TokenBank.from_state_dict(bank.state_dict(), 'cuda')
    far = cand.clone()
    far[1, 2] = (1 << 32) + 3
    top = own.topk(qry, 5, T, cand=far.cuda())
    assert torch.equal(top[0], classes.long()) and torch.equal(top[1], values) and torch.equal(top[2], prob) and int(own.status_count) == 0
    with pytest.raises(ValueError, match='outside'):
        own.check()
    # a row of empty slots only: no finite entry, prob 0 everywhere
    none = _rerank(bank, qry, torch.full((5, 3), -1), 2)
    assert bool((none[0] == -1).all()) and bool(torch.isneginf(none[1]).all()) and bool((none[2] == 0).all()) and int(none[5]) == 0
    for tries in (-2, 1 << 30):
        assert int(_rerank(bank, qry, torch.full((5, 1), tries), 1)[5]) == 5


def test_rerank_refusals_launch_nothing():
    case, bank, qry, dense = _bank((12, 3, 5, 25, 64, 25))
    with pytest.raises(ValueError):
        _rerank(bank, qry, torch.zeros(5, 3, dtype=torch.int64), 4)                 # k > M
    with pytest.raises(ValueError):
        _rerank(bank, qry, torch.zeros(5, 33, dtype=torch.int64), 4)                # M > 32
    ops = _ops()
    xhat, pooled = torch.empty_like(qry), torch.empty(5, 64, device='cuda')
    ops.emd_table_prep(qry, xhat, pooled)
    m = bank.class_maps()
    with pytest.raises(ValueError, match='temperature'):
        ops.emd_rerank((qry, xhat, pooled), (m[0], m[1], m[2], m[4]), torch.zeros(5, 3, dtype=torch.int32, device='cuda'), float('nan'), 2)
    out = ops.emd_rerank((qry[:0], xhat[:0], pooled[:0]), (m[0], m[1], m[2], m[4]), torch.zeros(0, 3, dtype=torch.int32, device='cuda'), T, 2)      # Q == 0
    assert out[0].shape == (0, 2) and int(out[4]) == 0 and int(out[5]) == 0


# ---------------------------------------------------------------- 3. re-rank against float64
@pytest.mark.parametrize('key', [(12, 3, 5, 7, 64, 7), (12, 3, 5, 25, 64, 25), (40, 3, 5, 7, 64, 3)])
def test_rerank_matches_the_float64_oracle(key):
    """values: within 1e-4 of the oracle logit of their class (the bound of tests/test_gpu_emd.py for one problem; 1.2e-6 measured there).
    Sortedness: oracle[returned class at rank r] >= (r-th largest oracle logit over the candidates) - 2e-4: two logits the GPU orders the other way
    round differ by at most 2 * 1e-4 in the oracle, so the check holds under near-ties and skips no row.
    prob against the float64 softmax of the returned values: exp(v - max) of a term has the absolute error e * (|v - max| 2^-24 + 2 ulp) <=
    0.37 * 2^-24 + 2^-22 = 2.6e-7 (x exp(-x) <= 0.37), the sum of at most 32 terms <= 1 each adds 6 tree levels of 2^-24 relative and the terms'
    own error, the division 2^-24: at most about 1e-6 on a probability <= 1; with a margin of 3 and rounded up, 1e-5."""
    case, bank, qry, dense = _bank(key)
    _, oracle = bc.bank_oracle(key)
    n_classes, Q = key[0], key[2]
    M = min(32, n_classes)
    g = torch.Generator().manual_seed(key[3])
    cand = torch.stack([torch.randperm(n_classes, generator=g)[:M] for _ in range(Q)])
    classes, values, prob, _ = (t.cpu() for t in _rerank(bank, qry, cand, M, want_logits=True)[:4])
    assert sorted(classes[0].tolist()) == sorted(cand[0].tolist())
    want = torch.gather(oracle, 1, classes.long())
    finite = torch.isfinite(want)
    assert torch.equal(torch.isfinite(values), finite)
    err = (values.double() - want)[finite].abs().max().item()
    ranked = torch.gather(oracle, 1, cand).sort(dim=-1, descending=True).values
    slack = (ranked - want)[finite].max().item()
    soft = torch.softmax(values.double(), dim=-1)
    perr = (prob.double() - soft).abs().max().item()
    print(f'emd_rerank {key}: max |value - oracle| = {err:.3e}, worst order slack = {slack:.3e}, max |prob - softmax| = {perr:.3e}')
    assert err <= 1e-4
    assert bool((want >= ranked - 2e-4)[finite].all()) and bool((~finite == torch.isneginf(ranked)).all())
    assert perr <= 1e-5 and bool((prob[~finite] == 0).all())


# ---------------------------------------------------------------- 4. the module
def _model(**kw):
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    models.register(ENCODER)(lambda **a: Visformer(**TINY, **a))
    torch.manual_seed(3)
    return models.make('deepemd', encoder=ENCODER, encoder_args={'numerics': 'parity'}, **kw).cuda().eval()


def _stable_topk(logits, k):
    order = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :k]
    return order, torch.gather(logits, 1, order)


def test_fit_predict_and_predict_topk():
    m = _model()
    g = torch.Generator().manual_seed(11)
    xs, ys = torch.randn(7, 3, 80, 80, generator=g).cuda(), torch.tensor([2, 0, 2, 3, 0, 2, 3]).cuda()      # 4 classes, class 1 without examples
    xq = torch.randn(5, 3, 80, 80, generator=g).cuda()
    bank = m.fit(xs, ys, n_classes=4)
    assert (bank.N, bank.C) == (25, 128) and bank.counts.tolist() == [2, 0, 3, 2]
    split = m.fit(xs[4:], ys[4:], bank=m.fit(xs[:4], ys[:4], n_classes=4))
    assert torch.equal(split.sum, bank.sum) and torch.equal(split.count, bank.count)
    logits = m.predict(bank, xq)
    assert logits.shape == (5, 4) and torch.equal(logits, bank.logits(m.encode(xq, False), m.temperature))
    assert bool(torch.isneginf(logits[:, 1]).all()) and bool(torch.isfinite(logits[:, [0, 2, 3]]).all())
    for k, shortlist in ((2, None), (4, 4), (3, 7)):                               # shortlist >= n_classes: all classes are re-ranked
        classes, values, prob = m.predict_topk(bank, xq, k, shortlist)
        ref_c, ref_v = _stable_topk(logits, k)
        assert torch.equal(classes, ref_c) and torch.equal(values, ref_v), (k, shortlist)
        full = torch.softmax(logits.double(), dim=-1)
        assert (prob.double() - torch.gather(full, 1, ref_c)).abs().max().item() <= 1e-5
    m.check_status()
    bank.check()
    # the stored bank round-trips
    from fewshot_vit_amd.models.emd_bank import TokenBank
    again = TokenBank.from_state_dict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in bank.state_dict().items()}, 'cuda')
    assert torch.equal(m.predict(again, xq), logits)
    with pytest.raises(ValueError):
        TokenBank(4, 25, 64, 'cuda').load_state_dict(bank.state_dict())
    with pytest.raises(ValueError, match='outside'):
        m.fit(xs[:1], torch.tensor([4]).cuda(), bank=again).check()
    with pytest.raises(RuntimeError, match='eval-mode'):
        m.train().predict(bank, xq)
    m.eval()
    with pytest.raises(NotImplementedError):
        _model(deepemd='grid').fit(xs, ys)


# ---------------------------------------------------------------- 5. the command line
def _png(path, rng, cls, size):
    from PIL import Image
    base = np.zeros((size[1], size[0], 3))
    base[..., cls] = 160.0                                   # a colour per class under noise
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.clip(base + rng.normal(40.0, 30.0, base.shape), 0, 255).astype(np.uint8)).save(path)


def _tree(root):
    """the tree of test_gpu_predict_cli.py: support 1 / 2 / 4 images, more 2 / 0 / 3, five query images"""
    rng = np.random.default_rng(5)
    for c, (name, n) in enumerate(zip(CLASSES, (1, 2, 4))):
        for i in range(n):
            _png(os.path.join(root, 'support', name, f's{i}.png'), rng, c, (96 + 8 * i, 100))
    for c, (name, n) in enumerate(zip(CLASSES, (2, 0, 3))):
        for i in range(n):
            _png(os.path.join(root, 'more', name, f'm{i}.png'), rng, c, (90, 90))
    for i in range(5):
        _png(os.path.join(root, 'query', f'q{i}.png'), rng, i % 3, (120, 92))


def _images(paths):
    from fewshot_vit_amd.datasets.folder_datasets import ImageFolder
    return ImageFolder.from_files(paths, [0] * len(paths), 80, 91, 'cuda', cache_bytes=0).gather(list(range(len(paths))))


def test_predict_cli_with_the_deepemd_head(tmp_path):
    from fewshot_vit_amd import models, predict
    root = str(tmp_path)
    _tree(root)
    ck, ck_bare, ck_proto, bank_f, out_f, top_f = (os.path.join(root, n) for n in ('ck.pth', 'bare.pth', 'proto.pth', 'bank.pt', 'preds.csv', 'top.csv'))
    sd = _model().state_dict()
    torch.save({'model': 'deepemd', 'model_args': {'encoder': ENCODER, 'encoder_args': {}}, 'model_sd': sd}, ck)
    torch.save({'params': sd}, ck_bare)                                          # a SUN-D checkpoint: no model_args
    sup_d, more_d, qry_d = (os.path.join(root, n) for n in ('support', 'more', 'query'))
    base = ['--head', 'deepemd', '--numerics', 'parity']
    res = predict.main(['--load', ck, '--support', sup_d, '--query', qry_d, '--out', out_f, '--save-bank', bank_f] + base)
    assert res['classes'] == list(CLASSES) and res['bank'].counts.tolist() == [1, 2, 4]
    rows = list(csv.reader(open(out_f)))
    assert rows[0] == ['file', 'pred_class', 'logit_0', 'logit_1', 'logit_2'] and len(rows) == 1 + 5
    assert [os.path.basename(r[0]) for r in rows[1:]] == [f'q{i}.png' for i in range(5)]
    # DeepEMD.fit / predict on the same transformed images
    model = predict.load_deepemd(ck, numerics='parity').cuda().eval()
    sup, lab = predict.list_labelled(sup_d, list(CLASSES))
    more, more_lab = predict.list_labelled(more_d, list(CLASSES))
    assert lab == [0, 1, 1, 2, 2, 2, 2] and more_lab == [0, 0, 2, 2, 2]
    bank = model.fit(_images(sup), torch.tensor(lab).cuda(), n_classes=3)
    logits = model.predict(bank, _images([r[0] for r in rows[1:]])).cpu()
    got = torch.tensor([[float(v) for v in r[2:]] for r in rows[1:]], dtype=torch.float64).float()
    assert torch.equal(got, res['logits']) and torch.equal(res['logits'], logits)
    assert [int(r[1]) for r in rows[1:]] == logits.argmax(-1).tolist() == res['pred'].tolist()
    # --topk 2 --shortlist 3: the same predictions, the columns of the prototype head's --topk
    top = predict.main(['--load', ck, '--load-bank', bank_f, '--query', qry_d, '--topk', '2', '--shortlist', '3', '--out', top_f] + base)
    assert torch.equal(top['pred'], res['pred']) and torch.equal(top['topk_logits'], torch.sort(logits, dim=-1, descending=True, stable=True).values[:, :2])
    assert list(csv.reader(open(top_f)))[0] == ['file', 'pred_class', 'pred_name'] + [f'{h}_{i}' for i in range(2) for h in ('class', 'name', 'logit', 'prob')]
    # a stored bank extended with more/ = one fit over both folders
    ext = predict.main(['--load', ck, '--load-bank', bank_f, '--support', more_d, '--query', qry_d] + base)
    both = model.fit(_images(sup + more), torch.tensor(lab + more_lab).cuda(), n_classes=3)
    assert ext['bank'].counts.tolist() == [3, 2, 7] and torch.equal(ext['bank'].sum, both.sum)
    assert torch.equal(ext['logits'], model.predict(both, _images(ext['files'])).cpu())
    # a checkpoint without model_args needs --encoder, and then scores the same
    bare = predict.main(['--load', ck_bare, '--encoder', ENCODER, '--load-bank', bank_f, '--query', qry_d] + base)
    assert torch.equal(bare['logits'], res['logits'])
    with pytest.raises(SystemExit):
        predict.main(['--load', ck_bare, '--load-bank', bank_f, '--query', qry_d] + base)
    # the bank file records its head
    m = models.make('meta-baseline', encoder=ENCODER, encoder_args={})
    torch.save({'model': 'meta-baseline', 'model_args': {'encoder': ENCODER, 'encoder_args': {}}, 'model_sd': m.state_dict()}, ck_proto)
    with pytest.raises(ValueError, match='--head'):
        predict.main(['--load', ck_proto, '--load-bank', bank_f, '--query', qry_d, '--numerics', 'parity'])
    proto_bank = os.path.join(root, 'proto_bank.pt')
    predict.main(['--load', ck_proto, '--support', sup_d, '--save-bank', proto_bank, '--numerics', 'parity'])
    with pytest.raises(ValueError, match='--head'):
        predict.main(['--load', ck, '--load-bank', proto_bank, '--query', qry_d] + base)
