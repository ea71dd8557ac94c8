"""The host record of a generation's rules (decode.StepRules) and the search decoders' refusal tables, without a GPU: the defaults
are "off", a lane's record holds views of its own rows, and every setting a search refused before the tables existed is still
refused, with the same words, before anything of the decoder is read."""
import pytest
import torch

from mmtg_amd.constraints import MIROSTAT_OFF, WARP_OFF
from mmtg_amd.decode import BeamDecoder, ContrastiveDecoder, StepRules, StochasticBeamDecoder


def test_a_record_without_arguments_is_a_generation_without_rules():
    r = StepRules()
    for with_head in (True, False):
        assert r.forms(with_head) == ("", "", False) and r.forms(with_head, copies=True) == ("", "", False)
        assert r.key(with_head) == () == r.key(with_head, copies=True)
    assert r.warp == WARP_OFF and r.mirostat == MIROSTAT_OFF and r.groups == 1 and r.kw is None and not r.prefix
    fe = torch.zeros(4, dtype=torch.int32)
    assert r.tail(fe) == dict(fixed_end=None, ngram=0, tables=None, tmpl=None, rhyme=None, refrain=None)
    assert StepRules(prefix=True).tail(fe)["fixed_end"] is fe
    with pytest.raises(AttributeError):
        r.use_fixed = True                                                      # (slots: no loose attribute comes back)


def _full_record(B=4, n_lines=3, V=160):
    i = lambda dt, *s: torch.zeros(*s, dtype=dt)                                # noqa: E731
    lines = (i(torch.uint8, B, n_lines), i(torch.uint8, B, n_lines), i(torch.int32, 4, 5), i(torch.int16, B, n_lines))
    return StepRules(prefix=True, ngram=3, lines=lines, tmpl=i(torch.int32, B, n_lines, 20),
                     rhyme=(i(torch.int16, V), i(torch.int8, B, n_lines), True), refrain=i(torch.int8, B, n_lines),
                     warp=(0.05, 1.0, 0.0, 0.0), warp_src=i(torch.int8, B, n_lines), mirostat=(2.0, 0.1), return_logprobs=True)


def test_rows_gives_views_of_the_rows_and_the_shared_tables_themselves():
    B, a, z = 4, 2, 4
    r = _full_record(B)
    part = r.rows(a, z)
    lo, hi, sets, set_of = r.lines
    pairs = [(lo, part.lines[0]), (hi, part.lines[1]), (set_of, part.lines[3]), (r.tmpl, part.tmpl), (r.rhyme[1], part.rhyme[1]),
             (r.refrain, part.refrain), (r.warp_src, part.warp_src)]
    for whole, view in pairs:
        assert view.shape[0] == z - a and view.shape[1:] == whole.shape[1:]
        assert view.data_ptr() == whole.data_ptr() + a * whole.stride(0) * whole.element_size()
        assert view.untyped_storage().data_ptr() == whole.untyped_storage().data_ptr()
    assert part.lines[2] is sets and part.rhyme[0] is r.rhyme[0] and part.rhyme[2] is True
    for name in ("prefix", "ngram", "warp", "mirostat", "return_logprobs", "groups", "diversity_penalty", "kw"):
        assert getattr(part, name) == getattr(r, name), name
    whole = r.rows(0, B)
    for with_head in (True, False):
        for copies in (False, True):
            assert whole.key(with_head, copies) == r.key(with_head, copies) == part.key(with_head, copies)
            assert whole.forms(with_head, copies) == r.forms(with_head, copies)
    # absent tables stay absent; end sets may be absent inside line tables
    bare = StepRules(ngram=2, lines=(lo, hi, None, None)).rows(a, z)
    assert bare.lines[2] is None and bare.lines[3] is None and bare.lines[0].data_ptr() == lo[a:].data_ptr()
    assert (bare.tmpl, bare.rhyme, bare.refrain, bare.warp_src, bare.kw) == (None,) * 5
    assert StepRules().rows(a, z).lines is None


# what each search decoder refused when its refusals were functions with one parameter per setting, and the words it used
_SEARCH_DRAWS_NOTHING = {
    "warp": "a search draws nothing: min_p / typical_p / epsilon_cutoff / eta_cutoff shape the distribution a sampled generation draws "
            "from (GreedyDecoder / generate_samples), and no sampling runs inside a beam or contrastive search",
    "mirostat": "a search draws nothing: mirostat_tau / mirostat_eta steer the surprise of what a sampled generation draws "
                "(GreedyDecoder / generate_samples), and no sampling runs inside a beam or contrastive search"}
_CUTS = (dict(min_p=0.1), dict(typical_p=0.9), dict(epsilon_cutoff=0.01), dict(eta_cutoff=0.01))
_TAUS = (dict(mirostat_tau=2.0), dict(mirostat_tau=0.5, mirostat_eta=0.0))
_DRAWS = (dict(top_k=10), dict(top_p=0.7), dict(generator=object()))
REFUSED = {
    BeamDecoder: [(kw, _SEARCH_DRAWS_NOTHING["warp"]) for kw in _CUTS] + [(kw, _SEARCH_DRAWS_NOTHING["mirostat"]) for kw in _TAUS] + [
        (dict(return_logprobs=True), "beam search has no return_logprobs (the merge reorders rows after the selection); score the beams "
                                     "with generate.score_sequences")],
    ContrastiveDecoder: [(kw, _SEARCH_DRAWS_NOTHING["warp"]) for kw in _CUTS] + [(kw, _SEARCH_DRAWS_NOTHING["mirostat"]) for kw in _TAUS] + [
        (kw, "contrastive search is deterministic: it takes no sampling top_k / top_p / generator (its top_k is the decoder's, given at "
             "construction)") for kw in _DRAWS] + [
        (dict(diversity_penalty=1.0), "contrastive search has no diversity_penalty: there are no beam groups to keep apart"),
        (dict(keywords=[(5, 6)]), "contrastive search takes no keywords=: it keeps one hypothesis per prompt, and a keyword needs banks of "
                                  "beams to be carried in (BeamDecoder / generate_beams)"),
        (dict(num_beam_groups=2), "contrastive search has no num_beam_groups: its rows are one step's candidates, not beams to group"),
        (dict(return_logprobs=True), "contrastive search has no return_logprobs (the merge reorders rows after the selection); score the "
                                     "lyric with generate.score_sequences")],
    StochasticBeamDecoder: [
        (kw, "stochastic beam search samples from the whole processed distribution: min_p / typical_p / epsilon_cutoff / eta_cutoff "
             "would truncate it before the perturbation, which is not built (a sampled generation takes them: GreedyDecoder / "
             "generate_samples)") for kw in _CUTS] + [
        (kw, "stochastic beam search has no mirostat_tau / mirostat_eta: Mirostat adapts a cut per row and draw, and the rows here are "
             "reordered by the merge (GreedyDecoder / generate_samples take it)") for kw in _TAUS] + [
        (kw, "stochastic beam search takes no sampling top_k / top_p / generator: it samples from the whole processed distribution, and "
             "its noise comes from seed=") for kw in _DRAWS] + [
        (dict(keywords=[(5, 6)]), "stochastic beam search takes no keywords=: its rows are samples in draw order, not banks of beams to "
                                  "carry a keyword in (BeamDecoder / generate_beams)"),
        (dict(num_beam_groups=2), "stochastic beam search has no num_beam_groups / diversity_penalty: a penalty between groups would "
                                  "change the distribution the samples come from"),
        (dict(diversity_penalty=1.0), "stochastic beam search has no num_beam_groups / diversity_penalty: a penalty between groups would "
                                      "change the distribution the samples come from"),
        (dict(return_logprobs=True), "stochastic beam search has no return_logprobs (the merge reorders rows after the selection); score "
                                     "the samples with generate.score_sequences")]}
DEFAULTS = dict(keywords=None, num_beam_groups=1, return_logprobs=False, diversity_penalty=0.0, top_k=1, top_p=0.0, generator=None,
                min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, mirostat_tau=0.0, mirostat_eta=0.1)
# (BeamDecoder takes keywords / num_beam_groups / diversity_penalty itself, and never read the base signature's top_k / top_p / generator)
TABLE_NAMES = {BeamDecoder: {"return_logprobs", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "mirostat_tau", "mirostat_eta"},
               ContrastiveDecoder: set(DEFAULTS), StochasticBeamDecoder: set(DEFAULTS)}


@pytest.mark.parametrize("cls", [BeamDecoder, ContrastiveDecoder, StochasticBeamDecoder])
def test_every_setting_a_search_refused_is_still_refused_in_the_same_words(cls):
    assert {k for names, _, _ in cls._REFUSED for k in names} == TABLE_NAMES[cls]
    for kw, words in REFUSED[cls]:
        for call in (cls._refuse, lambda **s: cls.begin(None, {}, 8, **s), lambda **s: cls.generate(None, {}, 8, **s)):
            with pytest.raises(ValueError) as e:                                 # (self is None: nothing of it is read before the refusal)
                call(**kw)
            assert str(e.value) == words, kw
            with pytest.raises(ValueError) as e:                                 # among settings that are forwarded, too
                call(temperature=1.1, prefix=None, **kw)
            assert str(e.value) == words, kw


@pytest.mark.parametrize("cls", [BeamDecoder, ContrastiveDecoder, StochasticBeamDecoder])
def test_defaults_pass_the_refusals_and_an_unknown_keyword_is_a_type_error(cls):
    mine = {k: v for k, v in DEFAULTS.items() if k in TABLE_NAMES[cls]}
    assert cls._refuse() == {} == cls._refuse(**mine)
    for k, v in mine.items():
        assert cls._refuse(**{k: v}) == {}
    assert cls._refuse(mirostat_tau=0.0, mirostat_eta=0.5) == {}                  # eta alone turns nothing on
    rest = dict(temperature=1.1, repitition_penalty=1.5, use_graph=False, prefix=[[1, 5]], no_repeat_ngram_size=3, refrain_scheme="AA")
    assert cls._refuse(**rest, **mine) == rest                                   # what is not refused is what is forwarded
    for name in ("no_such_setting", "teacher", "tap", "return_everything"):
        for call in (cls._refuse, lambda **s: cls.begin(None, {}, 8, **s), lambda **s: cls.generate(None, {}, 8, **s)):
            with pytest.raises(TypeError, match=name):
                call(**{name: 1})
    with pytest.raises(ValueError, match="min_p"):                               # out of range is said first, by name
        cls._refuse(min_p=7.0)
    with pytest.raises(ValueError, match="mirostat_tau"):
        cls._refuse(mirostat_tau=77.0)
