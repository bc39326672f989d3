"""Record tests/golden/text_stack_launches.json.xz: the kernel-library calls of the MED text stack, call for call.

Run on a GPU, at the commit whose launch sequence is to be kept:

    python tests/golden/make_text_stack_launches.py

tests/test_text_stack_launches_gpu.py runs the same cases through the same recorder and asserts equal traces, so a change of
the host code (vidil_amd/med.py, decoding.py, blip.py, sentence.py) that is meant to leave the device work alone can show that it did: equal
traces are the same kernels on the same operands with the same aliasing, hence the same bits.

The recorder wraps every public function of ``vidil_amd.kernels`` (it still calls through) and notes, per call made from outside
that module: the function's name; every scalar argument by value; for every tensor argument — those inside the ``heads=`` /
``arena=`` / ``ln=`` / ``rln=`` containers included — dtype, shape, strides, storage offset and the ordinal of its storage in
first-use order; and the same for a tensor it returns.  Every tensor seen is kept alive until its case ends, so the allocator
cannot hand one address out twice.  A case that ends in a VidilHipError records the message as its last entry.

The cases drive public entry points only, on the small geometry of tests/test_forward_surface_gpu.py (hidden 256, 4 heads,
2 layers, encoder width 256) with random weights: the values do not matter, only the calls.
"""
import contextlib
import inspect
import json
import lzma
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(HERE, "text_stack_launches.json.xz")
DEV = "cuda"
W = 256                          # hidden size = encoder width of the small geometry
KINDS = ("split", "f32", "16")   # the attention kinds of the parity precision mode


class Recorder:
    def __init__(self):
        self.calls, self.keep, self.storages, self.depth = [], [], {}, 0

    def enc(self, x):
        if isinstance(x, torch.Tensor):
            self.keep.append(x)
            ordinal = self.storages.setdefault((str(x.device), x.untyped_storage().data_ptr()), len(self.storages))
            return ["tensor", str(x.dtype), list(x.shape), list(x.stride()), x.storage_offset(), ordinal]
        if x is None or isinstance(x, (bool, int, float, str)):
            return x
        if isinstance(x, dict):
            return {str(k): self.enc(v) for k, v in sorted(x.items())}
        if isinstance(x, (list, tuple)):
            return [self.enc(v) for v in x]
        return str(x) if isinstance(x, (torch.dtype, torch.device)) else type(x).__name__

    def wrap(self, name, f):
        sig = inspect.signature(f)

        def call(*a, **kw):
            if self.depth:                       # (a library function calling another: one call of the text stack)
                return f(*a, **kw)
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            entry = [name, self.enc(dict(bound.arguments))]
            self.calls.append(entry)
            self.depth += 1
            try:
                ret = f(*a, **kw)
            finally:
                self.depth -= 1
            entry.append(self.enc(ret) if isinstance(ret, (torch.Tensor, bool, tuple)) else None)
            return ret
        return call

    @contextlib.contextmanager
    def recording(self):
        from vidil_amd import kernels as K

        saved = {n: f for n, f in vars(K).items() if inspect.isfunction(f) and f.__module__ == K.__name__ and not n.startswith("_")}
        for n, f in saved.items():
            setattr(K, n, self.wrap(n, f))
        try:
            yield
        except K.VidilHipError as e:
            self.calls.append(["raised", str(e)])
        finally:
            for n, f in saved.items():
                setattr(K, n, f)


# ------------------------------------------------------------------------------------------------ models, inputs, switches
def small_cfg():
    from vidil_amd.med import BertConfig

    return BertConfig(hidden_size=W, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, vocab_size=512,
                      max_position_embeddings=64, encoder_width=W)


class Models:
    def __init__(self):
        from vidil_amd.med import BertLMHeadModel, BertModel
        from vidil_amd.sentence import SentenceConfig, SentenceEncoder

        torch.manual_seed(0)
        self.enc = BertModel(small_cfg()).to(DEV).eval()
        self.dec = BertLMHeadModel(small_cfg()).to(DEV).eval()
        self.sent = SentenceEncoder(SentenceConfig(vocab_size=300, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                                   intermediate_size=256, max_position_embeddings=66, max_seq_length=64)).to(DEV).eval()


def images(B, Te, parity=False):
    """Encoder states of B units: f16 [B*Te, W], or their [hi | lo | hi] rows [B*Te, 3W] for the parity mode."""
    from vidil_amd import kernels as K

    x = torch.randn(B * Te, W, device=DEV)
    return K.split3(x, torch.empty((B * Te, 3 * W), dtype=torch.float16, device=DEV)) if parity else x.half().contiguous()


def tokens(P, T, lens=None):
    ids = torch.randint(1, 500, (P, T), dtype=torch.int32, device=DEV)
    lens = [T - (3 * p) % T for p in range(P)] if lens is None else lens
    return ids, torch.tensor(lens, dtype=torch.int32, device=DEV)


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@contextlib.contextmanager
def parity(model, kind):
    from vidil_amd.packing import set_parity_attention, set_parity_mode

    set_parity_mode(True, model)
    set_parity_attention(kind, model)
    try:
        yield
    finally:
        set_parity_attention(None, model)
        set_parity_mode(False, model)


@contextlib.contextmanager
def images_per_launch(n):
    from vidil_amd.med import BertModel

    old = BertModel.MAX_IMAGES_PER_LAUNCH
    BertModel.MAX_IMAGES_PER_LAUNCH = n
    try:
        yield
    finally:
        BertModel.MAX_IMAGES_PER_LAUNCH = old


# ------------------------------------------------------------------------------------------------ the cases
def encode_case(form, fuse, Te=26, T=12):
    """BertModel.encode over 2 images: no cross / cross_index / cross_groups + cross_max_group / cross_kv_len."""
    def run(m, recording):
        enc16 = images(2, Te)
        with env(VIDIL_FUSE_LN=fuse), recording():
            if form == "none":
                m.enc.encode(*tokens(4, T), None)
            elif form == "index":
                m.enc.encode(*tokens(4, T), m.enc.project_cross_kv(enc16, 2, Te), cross_index=i32([0, 1, 1, 0]))
            elif form == "groups":          # (up to 3 pairs x T tokens per image: more than 32 query rows -> row-major values)
                m.enc.encode(*tokens(5, T), m.enc.project_cross_kv(enc16, 2, Te, v_rowmajor=3 * T > 32 or Te > 768),
                             cross_groups=i32([0, 2, 5]), cross_max_group=3)
            else:
                unit = i32([Te, Te - 6])
                m.enc.encode(*tokens(4, T), m.enc.project_cross_kv(enc16, 2, Te, kv_len=unit), cross_index=i32([0, 1, 1, 0]),
                             cross_kv_len=i32([Te, Te - 6, Te - 6, Te]))
    return run


def encode_cls_case(form, fuse, Te=17, T=12):
    def run(m, recording):
        enc16 = images(3, Te)
        with env(VIDIL_FUSE_LN=fuse), recording():
            if form == "vt_index":
                m.enc.encode_cls(*tokens(3, T), m.enc.project_cross_kv(enc16, 3, Te), cross_index=i32([2, 0, 1]))
            else:                           # row-major V + last_layer_vt, image-major groups (one image without a pair)
                cross = m.enc.project_cross_kv(enc16, 3, Te, v_rowmajor=True, last_layer_vt=True)
                kw = dict(cross_groups=i32([0, 2, 2, 5]), cross_max_group=3)
                if form == "groups_pair_text":
                    m.enc.encode_cls(*tokens(3, T), cross, pair_text=torch.tensor([0, 1, 2, 0, 1], device=DEV), **kw)
                else:
                    m.enc.encode_cls(*tokens(5, T), cross, **kw)
    return run


def session_case(tiled, fuse, B=2, Te=26, P=4, shared=True, block=None, kind=None):
    """DecoderSession: the prompt pass and two decode steps of 3 beams per image."""
    def run(m, recording):
        from vidil_amd.blip import DecoderSession

        nb = 3
        enc16 = images(B, Te, parity=kind is not None)
        rows = B if shared else B * nb
        prompt = torch.randint(1, 500, (rows * P,), dtype=torch.int32, device=DEV)
        tok = torch.randint(1, 500, (B * nb,), dtype=torch.int32, device=DEV)
        beam = (torch.arange(B * nb, device=DEV) // nb * nb).to(torch.int32)
        with contextlib.ExitStack() as stack:
            stack.enter_context(env(VIDIL_DECODE_FUSE_LN=fuse))
            if block is not None:
                stack.enter_context(images_per_launch(block))
            if kind is not None:
                stack.enter_context(parity(m.dec, kind))
            stack.enter_context(recording())
            sess = DecoderSession(m.dec, enc16, B, nb, 8, tiled_cross=tiled)
            sess.prefill(prompt, P, shared=shared)
            sess.step(tok, beam, P)
            sess.step(tok, beam, P + 1)
    return run


def score_case(form, fuse=None, kind=None):
    def run(m, recording):
        enc16 = images(2, 26, parity=kind is not None)
        ids, lens = tokens(4, 10, [10, 7, 3, 5])
        kw = dict(image_index=[0, 1, 1, 0]) if form != "groups" else dict(group_start=[0, 1, 4])
        if form == "kv_len":
            kw["cross_kv_len"] = [26, 20]
        with contextlib.ExitStack() as stack:
            stack.enter_context(env(VIDIL_DECODE_FUSE_LN=fuse))
            if kind is not None:
                stack.enter_context(parity(m.dec, kind))
            stack.enter_context(recording())
            m.dec.score(enc16, 2, ids.cpu(), lens.cpu(), prompt_length=1, **kw)
    return run


def start_logits_case(m, recording):
    enc16 = images(2, 26)
    with recording():
        m.dec.start_logits(enc16, 2, 5, cross_kv_len=[26, 20])


def forward_case(m, recording):
    """The HF-signature forwards (masked_pass): a mask with holes on both sides; the causal pass with a prefix mask."""
    ids = torch.randint(1, 500, (2, 12), device=DEV)
    mask = torch.ones(2, 12, dtype=torch.long, device=DEV)
    mask[0, 3] = mask[1, 9:] = 0
    enc = torch.randn(2, 26, W, device=DEV)
    emask = torch.ones(2, 26, dtype=torch.long, device=DEV)
    emask[1, 5] = 0
    with recording():
        m.enc(ids, attention_mask=mask, encoder_hidden_states=enc, encoder_attention_mask=emask, output_hidden_states=True)
        m.dec(ids, attention_mask=(torch.arange(12, device=DEV)[None, :] < i32([12, 7])[:, None]).long(), encoder_hidden_states=enc,
              labels=ids)


def long_keys_case(form, fuse=None, Te=800):
    """More than LONG_KEYS encoder states per unit."""
    def run(m, recording):
        enc16 = images(2, Te)
        with env(VIDIL_FUSE_LN=fuse), recording():
            if form == "encode_cls_groups":     # the last layer's one-row launch takes the bound for Nq = 1: max(3, 33)
                m.enc.encode_cls(*tokens(5, 12), m.enc.project_cross_kv(enc16, 2, Te, v_rowmajor=True, last_layer_vt=True),
                                 cross_groups=i32([0, 2, 5]), cross_max_group=3)
            else:                               # 12 query rows per unit on plain K / V: refused
                m.enc.encode(*tokens(4, 12), m.enc.project_cross_kv(enc16, 2, Te, v_rowmajor=True), cross_index=i32([0, 1, 1, 0]))
    return run


def parity_encode_case(kind, form):
    def run(m, recording):
        enc3 = images(2, 26, parity=True)
        kw = dict(cross_index=i32([0, 1, 1, 0])) if form == "index" else dict(cross_groups=i32([0, 2, 4]), cross_max_group=2)
        with parity(m.enc, kind), recording():
            cross = m.enc.project_cross_kv(enc3, 2, 26)
            m.enc.encode(*tokens(4, 12), cross, **kw)
            if kind != "16":
                m.enc.encode_cls_parity(*tokens(4, 12), cross, **kw)
    return run


def sentence_case(kind):
    """3 sentences of at most 6 tokens (kind "16" is refused: the bias table needs the f32-row attention)."""
    def run(m, recording):
        from vidil_amd.packing import set_parity_attention

        ids, lens = tokens(3, 6, [6, 4, 1])
        set_parity_attention(kind, m.sent)
        try:
            with recording():
                m.sent.hidden_states(ids, lens)
        finally:
            set_parity_attention("split", m.sent)
    return run


def search_owner(m, prompt):
    """A BLIP_Decoder that is nothing but what the beam search asks of its owner: text_decoder, the tokenizer's [SEP] / [PAD]
    ids and prompt_ids (no ViT, no real tokenizer)."""
    from vidil_amd.blip import BLIP_Decoder

    class Owner(BLIP_Decoder):
        def prompt_ids(self, B, device):
            return torch.tensor([prompt] * B, dtype=torch.int32, device=device)

    owner = Owner.__new__(Owner)
    torch.nn.Module.__init__(owner)
    owner.text_decoder = m.dec
    owner.tokenizer = types.SimpleNamespace(sep_token_id=2, pad_token_id=0)
    return owner


def search_case(calls=1, graphs=None, B=2, P=4, num_beams=3, **kw):
    """Whole beam searches through generate_ids, B images of 26 encoder rows: ``calls`` consecutive ones on one owner (the first
    runs plain launches, the second captures its steps — recorded while they are captured —, the third replays: prompt pass
    and beam_finalize only).  check_done_every=0: without the done-poll, the only branch that depends on timing and the only
    way into compaction, a search's calls depend neither on values nor on timing."""
    def run(m, recording):
        owner = search_owner(m, [5, 6, 7, 8][:P])
        enc16 = [images(B, 26) for _ in range(calls)]
        with env(VIDIL_DECODE_GRAPHS=graphs, VIDIL_DECODE_FUSE_LN=None), recording():
            for e in enc16:
                owner.generate_ids(e, B, num_beams=num_beams, max_length=8, min_length=3, check_done_every=0, **kw)
        if calls > 1 and not all(st["graphs_ok"] and st["graphs"] for st in owner._decode_state.values()):
            raise RuntimeError("the decode steps were not captured: this trace is not the capture / replay schedule")
    return run


def cases():
    c = {}
    for fuse in (None, "0"):
        tag = "" if fuse is None else ",fuse_ln=0"
        for form in ("none", "index", "groups", "kv_len"):
            c[f"encode[{form}{tag}]"] = encode_case(form, fuse)
        for form in ("vt_index", "groups_pair_text", "groups"):
            c[f"encode_cls[{form}{tag}]"] = encode_cls_case(form, fuse)
        # Te = 800 > LONG_KEYS: 3-token rows in groups, the bound rounded up to ceil(33 / 3); the one-row last layer; a refusal
        c[f"long_keys[encode_groups_3_tokens{tag}]"] = encode_case("groups", fuse, Te=800, T=3)
        c[f"long_keys[encode_cls_groups{tag}]"] = long_keys_case("encode_cls_groups", fuse)
        c[f"long_keys[encode_index_refused{tag}]"] = long_keys_case("index_refused", fuse)
        tag = "" if fuse is None else ",decode_fuse_ln=0"
        for tiled in (True, False):
            c[f"session[tiled={tiled}{tag}]"] = session_case(tiled, fuse)
            c[f"session[tiled={tiled},5_images_in_blocks_of_2{tag}]"] = session_case(tiled, fuse, B=5, block=2)
        c[f"session[one_token_prompt{tag}]"] = session_case(True, fuse, P=1)
        c[f"session[every_row_prefill{tag}]"] = session_case(False, fuse, shared=False)
        c[f"long_keys[tiled_session{tag}]"] = session_case(True, fuse, Te=800)
        for form in ("index", "groups", "kv_len"):
            c[f"score[{form}{tag}]"] = score_case(form, fuse)
    c["start_logits[kv_len]"] = start_logits_case
    c["forward[masks]"] = forward_case
    for kind in KINDS:
        for form in ("index", "groups"):
            c[f"parity[{kind},encode,{form}]"] = parity_encode_case(kind, form)
        for tiled in (True, False):
            c[f"parity[{kind},session,tiled={tiled}]"] = session_case(tiled, None, kind=kind)
        c[f"parity[{kind},session,tiled=True,5_images_in_blocks_of_2]"] = session_case(True, None, B=5, block=2, kind=kind)
        c[f"parity[{kind},score]"] = score_case("index", kind=kind)
        c[f"parity[{kind},sentence]"] = sentence_case(kind)
    c["search[eager]"] = search_case(graphs="0")
    c["search[eager,capture,replay]"] = search_case(calls=3)
    c["search[one_token_prompt]"] = search_case(P=1)                       # (the VQA form: the arena_prompt route)
    c["search[6_beams,penalty]"] = search_case(num_beams=6, repetition_penalty=1.2)   # (the wide selection kernel, seqs= / penalty=)
    c["search[streams=2]"] = search_case(B=4, streams=2)                   # (two parts of 2 images, stepped round robin)
    return c


def trace(run, models):
    """The recorded calls of one case, in the form the golden file holds them (JSON types)."""
    rec = Recorder()
    with torch.no_grad():
        run(models, rec.recording)
    torch.cuda.synchronize()
    return json.loads(json.dumps(rec.calls))


def load_golden():
    with lzma.open(GOLDEN, "rt") as f:
        return json.load(f)


def main():
    models = Models()
    out, broken = {}, []
    for name, run in cases().items():
        try:
            out[name] = trace(run, models)
        except (ValueError, TypeError, NotImplementedError, AttributeError) as e:   # a mistake in the case itself: show them all
            print(f"{name}: {type(e).__name__}: {e}", flush=True)
            broken.append(name)
            continue
        tail = out[name][-1]
        print(f"{name}: {len(out[name])} calls" + (f", refused: {tail[1][:90]}" if tail[0] == "raised" else ""), flush=True)
    if broken:
        sys.exit(f"nothing written: {len(broken)} cases failed")
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with lzma.open(path, "wt") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"{os.path.basename(path)}: {len(out)} cases, {sum(len(v) for v in out.values())} calls, {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
