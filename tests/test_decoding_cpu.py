"""vidil_amd/decoding.py without a device: the session cache's key, lookup and eviction on stand-in entries (plain dicts, as the
real ones are), and the structure the module exists for — one search object behind a generator without closures, and the
search inherited from BeamSearchMixin instead of borrowed."""
import inspect

from vidil_amd import decoding as D


def test_session_keys():
    shape = dict(nb=3, max_length=20, min_length=5, dev="cuda:0", Te=197, P=4, penalty=1.0)
    main = D.session_key(8, slot=1, **shape)
    assert main[0] == 8 and main[-1] == 1
    assert D.session_key(8, slot=1, compact=True, **shape)[-1] == ("compact", 1)
    assert D.session_key(8, slot=1, compact=True, **shape)[:-1] == main[:-1]
    assert D.session_key(8, slot=0, **shape) != main                                    # only the slot differs
    assert D.session_key(8, slot=1, **dict(shape, penalty=1.2)) != main                 # only the repetition penalty differs
    assert D.session_key(8, slot=1, **shape) == main


def test_lookup_wants_the_identical_packed_weights():
    a, b = [1.0], [2.0]
    entry = dict(packs=(a, b))
    cache = {"k": entry}
    assert D.session_lookup(cache, "k", (a, b)) is entry
    assert D.session_lookup(cache, "k", (a, [2.0])) is None and D.session_lookup(cache, "k", ([1.0], b)) is None    # equal, not identical
    assert D.session_lookup(cache, "other", (a, b)) is None


def _main(i):
    return (i, 3, 20, 5, "cuda:0", 197, 4, 1.0, 0)


def test_make_room_drops_the_compact_sessions_first():
    cache = {_main(i): dict(last_used=i) for i in range(1, 6)}
    cache.update({_main(i)[:-1] + (("compact", 0),): dict(last_used=0) for i in (11, 12, 13)})
    assert len(cache) == D.MAX_SESSIONS == 8
    D.session_make_room(cache)
    assert sorted(cache) == [_main(i) for i in range(1, 6)]


def test_make_room_drops_the_least_recently_used_until_seven_remain():
    cache = {_main(i): dict(last_used=i) for i in range(1, 9)}
    del cache[_main(5)]["last_used"]                          # counts as 0: the first to go
    D.session_make_room(cache)
    assert sorted(k[0] for k in cache) == [1, 2, 3, 4, 6, 7, 8]
    D.session_make_room(cache)                                # 7 entries: there is room
    assert len(cache) == 7
    # the order in which entries leave: missing (0), then ascending last_used
    cache = {_main(i): dict(last_used=i) for i in range(1, 11)}
    del cache[_main(7)]["last_used"]
    D.session_make_room(cache)
    assert sorted(k[0] for k in cache) == [3, 4, 5, 6, 8, 9, 10]
    few = {_main(1): dict(last_used=1), _main(2)[:-1] + (("compact", 0),): {}}
    D.session_make_room(few)                                  # below the limit nothing leaves, compact sessions included
    assert len(few) == 2


def test_the_search_is_one_object_and_is_inherited():
    from vidil_amd.blip import BLIP_Decoder, BLIP_Video_Decoder
    from vidil_amd.blip_vqa import BLIP_VQA, BLIP_Video_VQA

    src = inspect.getsource(D.BeamSearchMixin._beam_search)
    assert "nonlocal" not in src and src.count("def ") == 1                              # no nested def
    assert "generate_ids" not in BLIP_VQA.__dict__ and "_beam_search" not in BLIP_VQA.__dict__
    assert BLIP_VQA.generate_ids is BLIP_Decoder.generate_ids is D.BeamSearchMixin.generate_ids
    assert BLIP_VQA._beam_search is BLIP_Decoder._beam_search
    for cls in (BLIP_Decoder, BLIP_Video_Decoder, BLIP_VQA, BLIP_Video_VQA):
        assert issubclass(cls, D.BeamSearchMixin)
    assert "sample_ids" in BLIP_Decoder.__dict__ and not hasattr(BLIP_VQA, "sample_ids")
    for name in ("text_decoder", "tokenizer.sep_token_id", "tokenizer.pad_token_id", "prompt_ids(B, device)"):
        assert name in D.BeamSearchMixin.__doc__                                          # the owner contract is written down


def test_blip_still_exports_the_session_and_the_trace():
    from vidil_amd import blip

    assert blip.DecoderSession is D.DecoderSession and blip.DecodeTrace is D.DecodeTrace
