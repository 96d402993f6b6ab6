"""No GPU: csrc/decoder_plan.hpp, the value that says what one row chunk of the decoder launches (plan_chunk), apart from the code
that launches it.  tests/decoder_plan_main.cpp is compiled with g++ and the address / undefined-behaviour sanitizers (a plain
executable: nothing is preloaded) and run twice:

  * over its whole enumeration of inputs, every plan held to the invariants of the header (the runs tile the blocks, the cross
    layers in order, every lin_z term delivered exactly once, no buffer overwritten unread or read unwritten, ...); the case
    count it prints is recomputed here from the enumeration rule;
  * with --layouts, printing the plans of given inputs as text.  Those are compared with `restated_plan` below -- the routing loop
    of decoder_forward as it stood before the plan was split off, restated statement by statement in Python, which is what
    tests/golden/decoder_plan_layouts.txt was written from (regenerate: python tests/test_decoder_plan_host.py) -- over a sample
    of the enumeration, and with the fixture for decoder_layout_cases.PRODUCT_LAYOUTS under the default flags.  A routing change
    shows up as a diff of that file.  The restatement itself is held to the same invariants (check_plan)."""
import itertools
import math
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT           # (first: it puts the repository on the path)
import decoder_layout_cases as dc

FIXTURE = os.path.join(GOLDEN, 'decoder_plan_layouts.txt')
STANDALONE, SEPARATE = 512, 1024           # OCC4D_LINZ_PATH_STANDALONE, OCC4D_CHAIN_PATH_SEPARATE
CHAIN_BLOCKS = 3
# (resblock, trunk4, x6trunk, f16block) as decoder_layout can produce them
FAMILIES = [(0, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 1)]
DEFAULTS = dict(flags=0, penult=0, k_local=8, chain_tail=1, one_pass=1, resblock=1, trunk4=0, x6trunk=0, f16block=0,
                H=416, m=40, c=130, D=416)


def make_inputs(name, n_blocks, cross_after, **kw):
    i = dict(DEFAULTS, name=name, nB=n_blocks, cross_after=list(cross_after))
    i['post_ok'] = [1] * len(cross_after)
    i['tail_ok'] = [1] * len(cross_after)
    i.update(kw)
    return i


# ---------------------------------------------------------------------------------------------------------------- the restatement
def restated_plan(i):
    """The loop nest of decoder_forward before csrc/decoder_plan.hpp, decisions only: in_rowlin / as_dense, the runs, the pass
    slots, dense_free, the kernel ladder, the LinzTerms of the post Linear."""
    nB, ca, nC = i['nB'], i['cross_after'], len(i['cross_after'])
    linz = bool(not (i['flags'] & STANDALONE) and i['resblock'] and not i['trunk4'] and not i['x6trunk'] and not i['penult']
                and i['k_local'] == 8 and i['m'] * nB * i['H'] < 2 ** 30 and i['c'] * i['H'] < 2 ** 30)
    in_rowlin, as_dense = [False] * (nB + 3), [False] * (nB + 3)
    any_dense = False
    for j in range(nC if linz else 0):
        b = ca[j] + 1
        if b >= nB or not i['post_ok'][j]:
            continue
        in_rowlin[b] = True
        cross_behind_b = j + 1 < nC and ca[j + 1] == b
        if b + 1 < nB and not cross_behind_b:
            as_dense[b + 1] = any_dense = True
    chain = linz and not (i['flags'] & SEPARATE)
    runs, next_cross, first_block = [], 0, 0
    while first_block < nB:
        s = first_block

        def cross_behind(b):
            return next_cross < nC and ca[next_cross] == b
        e = s
        while chain and e - s + 1 < CHAIN_BLOCKS and e + 1 < nB and not cross_behind(e):
            e += 1
        nb, cross = e - s + 1, cross_behind(e)
        n_tail = 0
        if chain and i['chain_tail'] and cross and i['tail_ok'][next_cross] and i['one_pass']:
            n_tail = 2 * i['D']
        first = not in_rowlin[s] and not as_dense[s]
        addp = ['-'] * CHAIN_BLOCKS
        slot_term, slot_rows = [s if first else -1, -1, -1], ['x' if first else '-', '-', '-']
        dense_free = any_dense and not as_dense[s + 1]
        slots = fresh = 0
        for k in range(s, e + 1):
            if as_dense[k + 1]:
                addp[k - s] = 'dense'
                continue
            if k == e:
                continue
            if dense_free:
                rows = 'dense'
            else:
                rows, fresh = 'f%d' % fresh, fresh + 1
            dense_free = False
            slots += 1
            slot_term[slots], slot_rows[slots], addp[k - s] = k + 1, rows, rows
        pass_ = 'interp_dense' if slots else 'interp_add' if first else 'none'
        if nb > 1 or n_tail:
            kernel = 'chain'
        elif i['f16block']:
            kernel = 'f16_block'
        elif i['x6trunk']:
            kernel = 'split_pair'
        elif i['resblock']:
            kernel = 'resblock4' if i['trunk4'] else 'resblock_addrows' if addp[0] != '-' else 'resblock'
        else:
            kernel = 'generic_pair'
        post, layer = [-1, -1], -1
        if cross:
            layer, next_cross = next_cross, next_cross + 1
            if in_rowlin[e + 1]:
                post[0] = e + 1
                if as_dense[e + 2]:
                    post[1] = e + 2
        runs.append(dict(first=s, nb=nb, cross=layer, tail=n_tail, pass_=pass_, slot_term=slot_term, slot_rows=slot_rows,
                         fresh=fresh, addrows=addp, kernel=kernel, post=post))
        first_block = e + 1
    return dict(linz=linz, chain=bool(chain), any_dense=any_dense, runs=runs)


def plan_text(name, p):
    lines = ['%s: linz=%d chain=%d any_dense=%d runs=%d' % (name, p['linz'], p['chain'], p['any_dense'], len(p['runs']))]
    for r in p['runs']:
        slots = ' '.join('%d>%s' % ts for ts in zip(r['slot_term'], r['slot_rows']))
        lines.append('  blocks %d+%d cross=%d tail=%d pass=%s slots=[%s] fresh=%d addrows=[%s] kernel=%s post=[%d %d]'
                     % (r['first'], r['nb'], r['cross'], r['tail'], r['pass_'], slots, r['fresh'], ' '.join(r['addrows']),
                        r['kernel'], r['post'][0], r['post'][1]))
    return lines


def check_plan(i, p):
    """The invariants of check() in tests/decoder_plan_main.cpp, on a restated plan."""
    nB, ca = i['nB'], i['cross_after']
    delivered = [0] * (nB + 2)
    held = {}                                   # buffer name -> the term it holds, unread
    nxt = next_cross = 0
    assert p['linz'] or not (p['chain'] or p['any_dense'])
    for r in p['runs']:
        s, last = r['first'], r['first'] + r['nb'] - 1
        assert s == nxt and 1 <= r['nb'] <= CHAIN_BLOCKS and last < nB and (r['nb'] == 1 or p['chain'])
        assert not any(next_cross < len(ca) and ca[next_cross] == b for b in range(s, last))
        nxt = last + 1
        if next_cross < len(ca) and ca[next_cross] == last:
            assert r['cross'] == next_cross
            next_cross += 1
        else:
            assert r['cross'] == -1
        if r['tail']:
            assert p['chain'] and i['chain_tail'] and i['one_pass'] and r['cross'] >= 0 and i['tail_ok'][r['cross']]
            assert r['tail'] == 2 * i['D'] and r['kernel'] == 'chain'
        for slot, (t, where) in enumerate(zip(r['slot_term'], r['slot_rows'])):
            assert (t < 0) == (where == '-')
            if t < 0:
                continue
            if slot == 0:
                assert t == s and where == 'x'
                delivered[t] += 1
            else:
                assert s < t <= last and where not in held and (where != 'dense' or p['any_dense']), (where, held)
                held[where] = t
        want = 'interp_dense' if max(r['slot_term'][1:]) >= 0 else 'interp_add' if r['slot_term'][0] >= 0 else 'none'
        assert r['pass_'] == want
        for k, where in enumerate(r['addrows']):
            if where == '-':
                continue
            assert k < r['nb'] and r['kernel'] in ('chain', 'resblock_addrows') and held.get(where) == s + k + 1, (where, held)
            delivered[held.pop(where)] += 1
        assert set(held) <= {'dense'}, held
        if r['kernel'] == 'chain':
            assert p['chain'] and (r['nb'] > 1 or r['tail'])
        if r['post'][0] >= 0:
            assert p['linz'] and r['cross'] >= 0 and i['post_ok'][r['cross']] and r['post'][0] == last + 1 < nB
            delivered[r['post'][0]] += 1
        if r['post'][1] >= 0:
            assert r['post'][0] >= 0 and r['post'][1] == last + 2 < nB and p['any_dense'] and 'dense' not in held
            held['dense'] = r['post'][1]
        if not p['linz']:
            assert r['pass_'] == 'interp_add' and r['nb'] == 1 and not r['tail'] and not r['fresh'] and r['post'] == [-1, -1]
    assert nxt == nB and next_cross == len(ca) and not held
    assert delivered[:nB] == [1] * nB, delivered


# ---------------------------------------------------------------------------------------------------------------- the program
@pytest.fixture(scope='module')
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('decoder_plan') / 'decoder_plan_main')
    cmd = [shutil.which('g++') or 'g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'occlusions-4d_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'decoder_plan_main.cpp'), '-o', exe]
    subprocess.run(cmd, check=True)
    return exe


def input_line(i):
    nC = len(i['cross_after'])
    mask = lambda bits: sum(int(bool(b)) << j for j, b in enumerate(bits))       # noqa: E731
    fields = [i['name'], i['nB'], nC] + i['cross_after'] + [i[k] for k in ('flags', 'penult', 'k_local', 'chain_tail', 'one_pass',
                                                                         'resblock', 'trunk4', 'x6trunk', 'f16block')]
    return ' '.join(str(f) for f in fields + [mask(i['post_ok']), mask(i['tail_ok'])])


def printed_plans(program, inputs):
    run = subprocess.run([program, '--layouts'], input='\n'.join(input_line(i) for i in inputs) + '\n', capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    return run.stdout.splitlines()


def product_inputs():
    """decoder_layout_cases.PRODUCT_LAYOUTS under the default flags, as forward_output_only runs them and with the penult output."""
    out = []
    for name in dc.PRODUCT_LAYOUTS:
        case = dc.BY_NAME[name]
        after = sorted(dc.live_map(case)) if case.ia['local_mode'] == 'attention' else []
        for penult in (0, 1):
            out.append(make_inputs('%s/penult=%d' % (name, penult), case.ia['n_blocks'], after, penult=penult))
    return out


def sample_inputs():
    """Every position set of the enumeration x the 64 settings of its switches x the six kernel families, the per-layer bools
    stepping through their combinations."""
    out = []
    for nB in range(1, 7):
        for nC in range(0, min(4, nB) + 1):
            for after in itertools.combinations(range(nB), nC):
                for bits, (fam, family) in itertools.product(range(64), enumerate(FAMILIES)):
                    ok = (len(out) * 7 + bits + fam) % 4 ** nC
                    out.append(make_inputs(
                        's%d' % len(out), nB, after, flags=(STANDALONE if bits & 1 else 0) | (SEPARATE if bits & 2 else 0),
                        penult=bits >> 2 & 1, k_local=7 if bits & 8 else 8, chain_tail=bits >> 4 & 1, one_pass=bits >> 5 & 1,
                        resblock=family[0], trunk4=family[1], x6trunk=family[2], f16block=family[3],
                        post_ok=[ok >> 2 * j & 1 for j in range(nC)], tail_ok=[ok >> (2 * j + 1) & 1 for j in range(nC)]))
    return out


def test_every_enumerated_plan_holds_the_invariants(program):
    run = subprocess.run([program], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    positions = sum(math.comb(nB, nC) * 4 ** nC for nB in range(1, 7) for nC in range(0, min(4, nB) + 1))
    assert positions == 8266
    assert run.stdout.split() == ['cases', str(positions * len(FAMILIES) * 4 * 2 * 2 * 2 * 2)]


def test_the_restatement_holds_the_invariants_and_is_the_fixture():
    for i in product_inputs() + sample_inputs():
        check_plan(i, restated_plan(i))
    broken = restated_plan(make_inputs('b6c2', 6, [2, 4]))
    broken['runs'][1]['addrows'][0] = '-'                     # block 3 no longer adds the term of block 4
    with pytest.raises(AssertionError):
        check_plan(make_inputs('b6c2', 6, [2, 4]), broken)
    with open(FIXTURE) as f:
        assert f.read().splitlines() == fixture_lines()


def test_plans_equal_the_restated_loop(program):
    inputs = sample_inputs()
    assert len(inputs) == 118 * 64 * 6
    want = [line for i in inputs for line in plan_text(i['name'], restated_plan(i))]
    assert printed_plans(program, inputs) == want


def test_product_layout_plans_are_the_fixture(program):
    with open(FIXTURE) as f:
        assert printed_plans(program, product_inputs()) == f.read().splitlines()


def test_the_published_layout_routes_as_documented():
    """b6c2 (cross layers behind blocks 2 and 4), worked by hand from DESIGN.md 6: one joint pass, chains 0-2 and 3-4 with the query
    projections as tails, terms 3 and 5 in the post Linears, term 4 through the dense buffer."""
    p = restated_plan(make_inputs('b6c2', 6, [2, 4]))
    assert [(r['first'], r['nb'], r['cross'], r['kernel']) for r in p['runs']] == [(0, 3, 0, 'chain'), (3, 2, 1, 'chain'), (5, 1, -1, 'resblock')]
    assert [r['pass_'] for r in p['runs']] == ['interp_dense', 'none', 'none'] and p['runs'][0]['slot_term'] == [0, 1, 2]
    assert [r['post'] for r in p['runs']] == [[3, 4], [5, -1], [-1, -1]] and [r['tail'] for r in p['runs']] == [832, 832, 0]


def fixture_lines():
    return [line for i in product_inputs() for line in plan_text(i['name'], restated_plan(i))]


if __name__ == '__main__':
    with open(FIXTURE, 'w') as f:
        f.write('\n'.join(fixture_lines()) + '\n')
