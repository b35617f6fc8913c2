"""merge_species.py on the GPU box at the borders of its kernels and of its writer: every case of tests/merge_species_cases.py
through Context.species_merge, in every form the case names (LDS rows and long rows, one group and a group per file, one and two
writer threads), held to the sequential model (tests/merge_species_model.py) as tests/test_gpu_merge_species.py holds its random
cases -- the three matrices, means, medians and their rounded values as bit patterns, prevalence, order, the four files byte for
byte -- and the refusals by reason, sample, line and message.  tests/test_merge_species_cases_host.py shows, without a device,
that each case sits on the border it names."""
import os

import pytest

from midas_amd import abi
from tests import merge_species_cases as K
from tests import merge_species_model as M
from tests.test_gpu_merge_species import NAMES, bits, files_of, same

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered")]      # (np.median of 1e308 and 1.7e308 is inf, and says so)

CELL_COLUMN = {7: 'count_reads', 8: 'coverage', 9: 'relative_abundance'}


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def written(root, c):
    """The case's profiles as files (bytes as they stand, no newline of ours) -> their paths."""
    paths = []
    for s, text in zip(c['sample_ids'], c['profiles']):
        os.makedirs(os.path.join(str(root), s, 'species'))
        paths.append(os.path.join(str(root), s, 'species', 'species_profile.txt'))
        with open(paths[-1], 'wb') as handle:
            handle.write(text.encode())
    return paths


def held_to_the_model(ctx, tmp_path, c):
    want = K.expect(c)
    paths = written(tmp_path / 'in', c)
    if c['refused']:
        path, text = paths[want.sample], c['profiles'][want.sample]
        for kw, _ in c['forms']:
            with pytest.raises(abi.MidasSnpsError) as e:
                ctx.species_merge(paths, c['ids'], c['sample_depth'], **kw)
            assert e.value.bad[:2] == (want.reason, want.sample), (kw, e.value.bad, e.value.message)
            assert e.value.message.startswith(path)
            if want.reason == M.MISSING:
                assert "species '%s' of species_info.txt has no line" % want.what in e.value.message
                continue
            assert e.value.bad[2] == want.line and '%s line %d: ' % (path, want.line) in e.value.message
            species = text.split('\n')[want.line - 1].split('\t')[0]
            if want.reason < M.UNKNOWN:
                assert want.line == 1 and "the header has no column '%s'" % M.COLUMNS[want.reason - 1] in e.value.message
            elif want.reason == M.UNKNOWN:
                assert species == c.get('intruder', species) and "species '%s' is not in species_info.txt" % species in e.value.message
            else:
                assert "%s of species '%s' is not a number" % (CELL_COLUMN[want.reason], species) in e.value.message
        return
    seen = []
    for k, (kw, lds) in enumerate(c['forms']):
        with ctx.species_merge(paths, c['ids'], c['sample_depth'], **kw) as res:
            assert res.lds_rows == lds, kw
            assert res.groups == (len(paths) if kw.get('chunk_bytes') == 16 else 1)
            same(res, want)
            if c.get('side_cells'):
                assert res.side_cells > 0
            for threads in c.get('write_threads', (0,)):
                assert files_of(res, tmp_path / ('out_%d_%d' % (k, threads)), c['sample_ids'], threads) == want['files'], (kw, threads)
            seen.append([bits(getattr(res, n)) for n in NAMES] + [bits(res.rounded[n]) for n in NAMES] + [res.order.tolist()])
    assert all(x == seen[0] for x in seen)


@pytest.mark.parametrize("name", K.names('rows'))
def test_rows_up_to_the_largest_sorted_in_lds(ctx, tmp_path, name):
    held_to_the_model(ctx, tmp_path, K.named(name))


@pytest.mark.parametrize("name", K.names('switch'))
def test_the_two_forms_at_their_switch(ctx, tmp_path, name):
    held_to_the_model(ctx, tmp_path, K.named(name))


@pytest.mark.parametrize("name", K.names('rowsof'))
def test_designed_rows_in_both_forms(ctx, tmp_path, name):
    held_to_the_model(ctx, tmp_path, K.named(name))


@pytest.mark.parametrize("name", K.names('round'))
def test_values_on_the_halves_of_round(ctx, tmp_path, name):
    c = K.named(name)
    held_to_the_model(ctx, tmp_path, c)
    text = open(os.path.join(str(tmp_path), 'out_0_0', 'species_prevalence.txt')).read()
    assert '\t-0.0\t' in text and '\tinf\t' in text and text == K.expect(c)['files']['species_prevalence.txt']


@pytest.mark.parametrize("name", K.names('prev'))
def test_prevalence_at_both_ends_and_the_stable_order(ctx, tmp_path, name):
    held_to_the_model(ctx, tmp_path, K.named(name))


@pytest.mark.parametrize("name", K.names('table'))
def test_lookup_chains_and_ids_that_are_refused(ctx, tmp_path, name):
    held_to_the_model(ctx, tmp_path, K.named(name))


@pytest.mark.parametrize("name", K.names('fields'))
def test_fields_on_every_residue_and_line_shape(ctx, tmp_path, name):
    held_to_the_model(ctx, tmp_path, K.named(name))


@pytest.mark.parametrize("name", K.names('write'))
def test_the_writer_in_two_waves_and_in_one(ctx, tmp_path, name):
    held_to_the_model(ctx, tmp_path, K.named(name))
