"""Device-resident decoding of the MED text decoder: ``DecoderSession`` (cross K/V, the self-attention KV arena and the two
forward entry points), the per-shape cache of sessions with their captured decode-step graphs, one running beam search
(``BeamSearch``) and ``BeamSearchMixin``, which gives a model ``generate_ids``.

The whole beam search (log-softmax, EOS ban, top-2k, BeamSearchScorer bookkeeping, KV-cache reorder) runs on the device;
the host only enqueues kernels and reads the final token ids back once per batch.
"""
from __future__ import annotations

import os
import warnings

import torch

from . import kernels as K
from .med import BeamArena, CrossKV
from .packing import require_cuda


class DecodeTrace:
    """Optional capture of per-step tensors for parity tests (off on the hot path)."""

    def __init__(self):
        self.logits = []       # f32 [R,V] per forward
        self.cand_scores = []
        self.cand_index = []
        self.scores = None     # f32 [B]: the winning hypothesis' score (sum of log-probabilities / length) as the search reports it


class DecoderSession:
    """Device-resident decoding state of R = B*nb sequences over B images: per-image cross K/V (projected
    once), the append-only self-attention KV arena + ancestry table, and the two forward entry points the beam
    loop needs."""

    def __init__(self, text_decoder, enc16, B, nb, max_length, tiled_cross=False):
        """tiled_cross: keep the image K/V in fragment tiles (BertModel.project_cross_kv(tiled=True)) — every decode
        step streams them from HBM once, in whole KiB per wave load; the caller guarantees that no launch has more
        than 32 query rows per image (nb beams x 1 token, or the prompt's tokens)."""
        self.dec, self.bert = text_decoder, text_decoder.bert
        cfg = text_decoder.config
        dev = enc16.device
        self.B, self.nb, self.R = B, nb, B * nb
        self.H, self.L = cfg.num_attention_heads, cfg.num_hidden_layers
        Te = enc16.shape[0] // B
        self.tiled_cross = tiled_cross
        self.cross = self.bert.project_cross_kv(enc16, B, Te, tiled=tiled_cross)
        self.Tcap = max_length
        # (parity precision mode with vidil_attention_f32: the self-attention K / V cache is f32 too)
        from .packing import parity_attention_f32
        arena_dtype = torch.float32 if (self.bert.parity and parity_attention_f32(self.bert)) else enc16.dtype
        self.arena = BeamArena(self.L, self.Tcap, self.R, cfg.hidden_size, dev, dtype=arena_dtype)
        self.ws_prefill, self.ws_step = {}, {}
        self.logits = None
        # round 6: the decoder's post-LN stack without LayerNorm launches (BertModel._run_layers_fused: raw sums + row partials
        # between the GEMMs, the LayerNorms folded into the consuming / residual GEMMs) — a property of the SESSION, never of its
        # size: a caption must not depend on how many images share its search ($VIDIL_DECODE_FUSE_LN=0: the unfused launches)
        self.fused_ln = self.bert.decoder_fused_ln(enc16.dtype)

    @classmethod
    def like(cls, parent, B):
        """A session for ``B`` images with the parent's geometry and EMPTY buffers (no projection): ``adopt`` fills it
        with the state of a subset of the parent's images in the middle of a search."""
        self = cls.__new__(cls)
        self.dec, self.bert = parent.dec, parent.bert
        self.B, self.nb, self.R = B, parent.nb, B * parent.nb
        self.H, self.L = parent.H, parent.L
        self.tiled_cross, self.Tcap = parent.tiled_cross, parent.Tcap
        pc = parent.cross
        self.cross = CrossKV(torch.empty((pc.k.shape[0], B) + tuple(pc.k.shape[2:]), dtype=pc.k.dtype, device=pc.k.device),
                             torch.empty((pc.vt.shape[0], B) + tuple(pc.vt.shape[2:]), dtype=pc.vt.dtype, device=pc.vt.device),
                             B, pc.Te, pc.NP, tiled=pc.tiled, Tk_cap=pc.Tk_cap, f32=pc.f32)
        pa = parent.arena
        self.arena = BeamArena(pa.L, pa.Tcap, self.R, pa.k.shape[-1], pa.k.device, dtype=pa.k.dtype)
        self.ws_prefill, self.ws_step = {}, {}
        self.logits = None
        self.fused_ln = parent.fused_ln
        return self

    def adopt(self, parent, images, n_pos):
        """Take over the search state of the parent's images ``images`` (int64 [B] on the device; entries may repeat:
        padding) after ``n_pos`` cached positions: their cross K/V, their rows of the K/V arena and their ancestry
        rows, with the slot numbers (= beam rows, always rows of the same image) renumbered."""
        nb = self.nb
        j = torch.arange(nb, device=images.device)
        rows = (images[:, None] * nb + j).view(-1)                                        # parent row of each new row
        shift = ((torch.arange(self.B, device=images.device) - images) * nb).repeat_interleave(nb).to(torch.int32)
        self.cross.k.copy_(parent.cross.k.index_select(1, images))
        self.cross.vt.copy_(parent.cross.vt.index_select(1, images))
        self.arena.k[:, :n_pos].copy_(parent.arena.k[:, :n_pos].index_select(2, rows))
        self.arena.v[:, :n_pos].copy_(parent.arena.v[:, :n_pos].index_select(2, rows))
        self.arena._cur = parent.arena._cur                                                # the orientation step graphs expect
        self.arena.anc[:, :n_pos] = parent.arena.anc.index_select(0, rows)[:, :n_pos] + shift[:, None]
        return rows, shift

    def rebind(self, enc16):
        """Start a new search on another batch of the same shape IN THE SAME BUFFERS (cross K/V re-projected in place,
        arena orientation reset): device addresses stay what the captured decode-step graphs recorded."""
        Te = enc16.shape[0] // self.B
        self.cross = self.bert.project_cross_kv(enc16, self.B, Te, out=self.cross, tiled=self.tiled_cross)
        self.arena._cur = 0

    def prefill(self, ids_i32, P, shared=False):
        """Prompt pass.  shared=False: ids_i32 int32 [R*P], every row decoded -> logits f32 [R,V] (what HF
        generate() does).  shared=True: ids_i32 int32 [B*P], ONE row per image -> logits f32 [B,V]: the nb beams of
        an image are identical until the first beam update (models/blip.py:130-138 repeats the same prompt and
        image nb times), so their prompt pass is computed once and its K/V are stored once (arena slot b*nb, which
        the ancestry rows of all nb beams point at)."""
        rows = self.B if shared else self.R
        h32, h16 = self.bert.embed(ids_i32, P, 0)
        # the prompt block attends to itself through one scratch K / V^T pair shared by all layers
        sk, sv, NPp = self.bert.scratch_kv(rows, P, h16.dtype, ids_i32.device)
        self.arena.init_prompt(P, self.nb if shared else 1)
        self.bert.run_layers(h32, h16, rows=rows, T=P, self_k=sk, self_vt=sv, t_off=0, Tk_cap=P, NPs=NPp, causal=True,
                             kv_len=None, cross=self.cross, cross_group=1 if shared else self.nb, ws=self.ws_prefill,
                             arena=self.arena, arena_slot_stride=self.nb if shared else 1, fused=self.fused_ln,
                             arena_prompt=(P == 1 and shared))   # (a shared one-token prompt is still a prompt block: slot b*nb)
        return self.dec.lm_logits(h16, rows, P, h32=h32)

    def step(self, next_tok_i32, beam_idx_i32, past_len):
        """Re-point the beams at their new histories (``beam_idx``: models/med.py:951-955 _reorder_cache, here a
        reorder of the ancestry table only), then one cached forward of the single new token at position
        ``past_len``.  Returns logits f32 [R,V]."""
        self.arena.reorder(beam_idx_i32, past_len)
        h32, h16 = self.bert.embed(next_tok_i32, 1, past_len)
        self.bert.run_layers(h32, h16, rows=self.R, T=1, self_k=None, self_vt=None, t_off=past_len, Tk_cap=self.Tcap,
                             NPs=0, causal=False, kv_len=None, cross=self.cross, cross_group=self.nb, ws=self.ws_step,
                             arena=self.arena, fused=self.fused_ln)
        self.logits = self.dec.lm_logits(h16, self.R, 1, out=self.logits, h32=h32)
        return self.logits


# ------------------------------------------------------------------------------------------------ the session cache
# Session state (KV arena, cross K/V, beam buffers) is kept per shape (and per stream slot) and reused by the next batch:
# besides saving the allocations it keeps every device address stable, which is what lets the decode steps — ~160 launches
# of 8-30 us kernels each, issued faster by the GPU than Python can enqueue them — be captured once into HIP graphs (one per
# step index: the position is baked into the launches) and replayed.  The cache is the owner's __dict__["_decode_state"]: a
# plain dict of plain dicts (``session_entry``), keyed by ``session_key``.
MAX_SESSIONS = 8


def session_key(B, nb, max_length, min_length, dev, Te, P, penalty, slot, compact=False):
    """Key of the session of B images on stream slot ``slot``; ``compact``: of the bucket of B images that a search on that
    slot moves its unfinished images to.  (``penalty``: the step graphs bake it into their launches.)"""
    return (B, nb, max_length, min_length, str(dev), Te, P, penalty, ("compact", slot) if compact else slot)


def session_entry(sess, packs, graphs_ok):
    """A new entry around the DecoderSession ``sess``, with the beam-search state of its B x nb rows."""
    return dict(sess=sess, bufs=K.BeamBuffers(sess.B, sess.nb, sess.Tcap, sess.arena.k.device), graphs={}, pool=None, calls=0,
                packs=packs, graphs_ok=graphs_ok, n_done_host=torch.zeros((1,), dtype=torch.int32, pin_memory=True))


def session_lookup(cache, key, packs):
    """The entry under ``key``, or None when there is none or its captured graphs hold the addresses of other packed weights
    than ``packs`` (the parameters changed since the capture, e.g. a checkpoint was loaded): the caller builds a new one."""
    st = cache.get(key)
    return st if st is not None and st["packs"][0] is packs[0] and st["packs"][1] is packs[1] else None


def session_make_room(cache):
    """Before a new main session: the compact sessions go first (each holds its own cross K/V, arena and step graphs —
    roughly +1.6x of a main session's memory over the four bucket sizes — and is cheap to rebuild); if that was not enough, the
    LEAST RECENTLY USED main sessions go, one at a time, until there is room — the sessions a pipeline alternates between keep
    their captured step graphs when an eighth shape shows up."""
    if len(cache) >= MAX_SESSIONS:
        for k in [k for k in cache if isinstance(k[-1], tuple)]:
            del cache[k]
    while len(cache) >= MAX_SESSIONS:
        del cache[min(cache, key=lambda k: cache[k].get("last_used", 0))]


# ------------------------------------------------------------------------------------------------ one search
class BeamSearch:
    """One running search of ``owner`` (see BeamSearchMixin) over B images: the session it drives — the full batch, or (after
    compaction) a smaller session that adopted the images that are still searching —, the result buffers of the images that
    left it, and the constants of the search.  Creating it takes the main session from the owner's cache (or builds it),
    binds it to ``enc16`` and resets the beam state."""

    def __init__(self, owner, enc16, B, *, num_beams, max_length, min_length, trace=None, check_done_every=2, slot=0,
                 compact_min=256, repetition_penalty=1.0):
        dec, bert = owner.text_decoder, owner.text_decoder.bert
        self.eos, self.pad = owner.tokenizer.sep_token_id, owner.tokenizer.pad_token_id
        dev = enc16.device
        self.nb = nb = num_beams
        self.V = dec.config.vocab_size
        self.max_length, self.min_length, self.trace, self.check_done_every = max_length, min_length, trace, check_done_every
        self.prompt = owner.prompt_ids(B, dev)
        self.P = P = self.prompt.shape[1]
        self.rp = rp = float(repetition_penalty)
        self.keyed = (nb, max_length, min_length, dev, enc16.shape[0] // B, P, rp, slot)   # session_key's arguments behind B
        self.cache = cache = owner.__dict__.setdefault("_decode_state", {})
        self.packs = packs = (dec.packed(), bert.packed())     # captured graphs hold the addresses of these packed weights
        key = session_key(B, *self.keyed)
        st = session_lookup(cache, key, packs)
        if st is None:
            session_make_room(cache)
            # (the shared prompt pass has P query rows per image, a decode step nb)
            st = cache[key] = session_entry(DecoderSession(dec, enc16, B, nb, max_length, tiled_cross=P <= 32 and nb <= 32), packs,
                                            os.environ.get("VIDIL_DECODE_GRAPHS", "1") != "0")
        else:
            st["sess"].rebind(enc16)
        owner.__dict__["_decode_clock"] = st["last_used"] = owner.__dict__.get("_decode_clock", 0) + 1
        st["calls"] += 1
        st["bufs"].reset(self.prompt)
        self.main = self.st = st
        self.sess, self.bufs, self.B = st["sess"], st["bufs"], B
        self.use_graphs = st["graphs_ok"] and trace is None and st["calls"] >= 2    # the first batch warms every kernel up
        self.final_tok = self.final_len = None
        self.orig = None                           # device int64: original image of each image of the current session
        self.probe = None                          # event behind the copy of the done counter that is under way
        # ---- finished images leave the batch (VIDIL_DECODE_COMPACT=0 switches it off) --------------------------------
        # Real captions end at different lengths; an image whose nb hypotheses are complete only burns rows.  When the
        # polled counter says the searching images fit the next smaller bucket (3/4, 1/2, 1/4, 1/8 of B, at least
        # `compact_min` images), they move to a session of that size: cross K/V, arena rows, ancestry rows and beam
        # state are gathered (a few ms at 1,500 images), the finished ones are finalised where they are.  A search is
        # per image and every kernel's arithmetic is independent of the batch around a row, so the tokens do not change.
        # The random-weight benchmark never triggers this (nothing finishes before the length limit).
        compact = compact_min > 0 and trace is None and os.environ.get("VIDIL_DECODE_COMPACT", "1") != "0"
        gran = 64 if compact_min >= 64 else 1                                   # bucket sizes in whole 64-image steps
        buckets = sorted({max(compact_min, -(-(B * f) // (8 * gran)) * gran) for f in (6, 4, 2, 1)}, reverse=True) if compact else []
        self.buckets = [b for b in buckets if b < B]

    def select(self, logits, c, beams_in_logits=None):
        """Candidate selection on the logits of the sequences of length c, then the beam update.  ``beams_in_logits=1``: the
        shared prompt pass, one row of logits per image."""
        bufs, trace = self.bufs, self.trace
        cs, ci = K.logsoftmax_topk(logits, bufs.beam_scores, self.B, self.nb, self.eos if c < self.min_length else -1,
                                   beams_in_logits=beams_in_logits, seqs=bufs.seqs if self.rp != 1.0 else None, cur_len=c,
                                   penalty=self.rp)
        if trace is not None:
            trace.logits.append(logits.clone()); trace.cand_scores.append(cs.clone()); trace.cand_index.append(ci.clone())
        K.beam_update(bufs, cs, ci, self.V, c, self.eos, self.pad)

    def step(self, c):
        """Decode step at length c: forward of the token appended last, candidate selection, beam update."""
        self.select(self.sess.step(self.bufs.next_tok, self.bufs.beam_idx, c - 1), c)

    def _after_replay(self):
        # a replayed step graph did the device work of BeamArena.reorder() and kernels.beam_update(); this is the host-side
        # half of both: the arena's orientation flips and the sequence buffers change roles
        self.sess.arena._cur ^= 1
        self.bufs.swap()

    def run_step(self, c):
        """Queue the step at length c: a replay of its graph, its capture and then the replay, or plain launches.  Returns
        False when the capture failed: graphs are then switched off for every session of the owner and the caller starts
        the search again."""
        g = self.st["graphs"].get(c) if self.use_graphs else None
        if g is not None:
            g.replay()
            self._after_replay()
        elif self.use_graphs:
            try:
                g = torch.cuda.CUDAGraph()
                # thread_local: other threads (the RCCL watchdog of a multi-GPU run) may touch the runtime meanwhile
                with torch.cuda.graph(g, pool=self.st["pool"], capture_error_mode="thread_local"):
                    self.step(c)
                self.st["pool"] = g.pool()
                self.st["graphs"][c] = g
                g.replay()            # capture records, replay executes (host-side state already advanced)
            except Exception as e:    # capture unsupported here: finish this batch with plain launches, loudly
                warnings.warn(f"vidil_amd: decode-step graph capture failed ({e!r}); continuing without graphs")
                torch.cuda.synchronize()
                for s_ in self.cache.values():
                    s_["graphs_ok"] = False
                    s_["graphs"].clear()
                return False
        else:
            self.step(c)
        return True

    def poll(self, c):
        """True when the search can stop before length c.  "Every image has its nb finished hypotheses"
        (BeamSearchScorer.is_done) is polled WITHOUT a host wait: the counter travels to pinned memory behind an event and is
        looked at when it has arrived.  A step queued after the last image finished changes nothing (finished images are
        skipped by beam_update, like process() skips done batches, and beam_finalize takes their stored hypotheses)."""
        if self.check_done_every and self.trace is None and c % self.check_done_every == 0:
            if self.probe is not None and self.probe.query():
                n_done = int(self.st["n_done_host"][0])
                self.probe = None
                if n_done == self.B:
                    return True
                if self.buckets and self.max_length - c >= 3 and any(self.B - n_done <= b < self.B for b in self.buckets):
                    self.retire_and_compact(c)
            if self.probe is None:
                self.st["n_done_host"].copy_(self.bufs.n_done, non_blocking=True)
                self.probe = torch.cuda.Event()
                self.probe.record()
        elif self.check_done_every and self.trace is not None and int(self.bufs.n_done.item()) == self.B:
            return True                      # parity traces stop exactly where the reference's loop stops
        return False

    def _finalize(self, c):
        """beam_finalize of the current session at length c, its images' rows written to the result buffers."""
        out_tok, out_len, out_score = K.beam_finalize(self.bufs, c, self.eos, self.pad)
        if self.final_tok is None:
            self.final_tok, self.final_len = out_tok, out_len
        else:
            self.final_tok[self.orig] = out_tok[:self.orig.numel()]
            self.final_len[self.orig] = out_len[:self.orig.numel()]
        return out_score

    def retire_and_compact(self, c):
        """Blocking: read the exact done mask, finalise everything into the result buffers, move the searching images
        into the largest bucket they fit.  Returns False when they do not fit a smaller bucket after all."""
        bufs, sess, main = self.bufs, self.sess, self.main
        active = (bufs.done == 0).nonzero().view(-1)                      # (host wait: exact state)
        A = int(active.numel())
        fit = [b for b in self.buckets if A <= b < self.B]
        if not fit or A == 0:
            return False
        Bp = fit[-1]
        images = torch.cat([active, active[-1:].expand(Bp - A)])           # padding: copies of the last one, marked done
        key = session_key(Bp, *self.keyed, compact=True)
        st2 = session_lookup(self.cache, key, self.packs)
        if st2 is None:
            st2 = self.cache[key] = session_entry(DecoderSession.like(main["sess"], Bp), self.packs, main["graphs_ok"])
        if st2.get("last_call") != main["calls"]:                           # one use per search of the parent
            st2["calls"] += 1
            st2["last_call"] = main["calls"]
        rows, shift = st2["sess"].adopt(sess, images, c)
        nb2 = st2["bufs"]
        if nb2.swapped != bufs.swapped:
            nb2.swap()                                                      # same buffer roles as the step graphs saw
        nb2.seqs.copy_(bufs.seqs.index_select(0, rows))
        nb2.beam_scores.copy_(bufs.beam_scores.index_select(0, rows))
        nb2.next_tok.copy_(bufs.next_tok.index_select(0, rows))
        nb2.beam_idx.copy_(bufs.beam_idx.index_select(0, rows) + shift)
        for name in ("done", "n_hyp", "hyp_score", "hyp_len", "hyp_tok", "worst"):
            getattr(nb2, name).copy_(getattr(bufs, name).index_select(0, images))
        nb2.done[A:] = 1
        nb2.n_done.fill_(Bp - A)
        # only now: beam_finalize ADDS the running beams of unfinished images to their hypothesis lists in place
        # (BeamSearchScorer.finalize does), which must not reach the copies made above; the state left behind in
        # the old session is dead — its next search starts with reset()
        self._finalize(c)
        self.orig = (torch.arange(self.B, device=active.device) if self.orig is None else self.orig).index_select(0, active)
        self.st, self.sess, self.bufs, self.B = st2, st2["sess"], nb2, Bp
        self.use_graphs = st2["graphs_ok"] and st2["calls"] >= 2
        return True

    def finish(self, c):
        """(tokens i32 [B, max_length], lens i32 [B]) of all images, in their original order."""
        out_score = self._finalize(c)
        if self.trace is not None:
            self.trace.scores = out_score     # (a traced search never compacts: one score per image)
        return self.final_tok, self.final_len


def _advance(g):
    """One ``next()`` of a search generator: None while the search runs, its (tokens, lens) when it has returned."""
    try:
        next(g)
    except StopIteration as done:
        return done.value


class BeamSearchMixin:
    """``generate_ids``: the device-resident beam search (per-shape DecoderSession cache, captured step graphs) for an
    nn.Module that has

      * ``text_decoder``: a BertLMHeadModel,
      * ``tokenizer.sep_token_id`` (ends a hypothesis) and ``tokenizer.pad_token_id`` (fills the rows behind it),
      * ``prompt_ids(B, device)`` -> int32 [B, P] on the device: the ids every sequence of the B images starts with.

    Nothing else of the host is read; the session cache lives in its ``__dict__["_decode_state"]``."""

    @torch.no_grad()
    def generate_ids(self, enc16, B, *, num_beams=3, max_length=30, min_length=10, trace: DecodeTrace = None,
                     check_done_every=2, streams=1, compact_min=256, repetition_penalty=1.0):
        """enc16: f16 [B*Te, width] image tokens of B images.  Returns (tokens i32 [B,max_length], lens i32 [B]):
        best hypothesis incl. the prompt, then [SEP] if it fits, then [PAD].

        ``streams`` > 1: the images are cut into that many contiguous parts whose searches run side by side on their
        own HIP streams (``_beam_search`` is a generator that yields after queueing each step; the parts are stepped
        round robin).  Measured at 3,072 images: 2 parts +0.2 %, 3 parts -1.4 %, 4 parts -3.8 % of the whole step — the
        ~160 launches of a decode step are short but each already covers the chip (decode time scales ~1/CUs under a
        CU mask), so the default stays 1; kept for small batches per part of a larger job.
        A search is per image, so the tokens do not depend on the split.

        ``repetition_penalty`` != 1.0 (models/blip.py:127,161; the captioning call site leaves it at 1.0): the candidate
        selection of every step penalises the log-probabilities of the tokens a beam already holds, prompt included
        (``vidil_logsoftmax_topk_penalty``; oracle/beam_ref.py ``repetition_penalty``)."""
        require_cuda(enc16, "BLIP_Decoder.generate")
        K.require_num_beams(num_beams, "generate")          # (1..K.MAX_BEAMS; refused here, not in the middle of a search)
        if not repetition_penalty > 0:
            raise ValueError(f"repetition_penalty must be a strictly positive float, got {repetition_penalty}")   # (HF's message)
        kw = dict(num_beams=num_beams, max_length=max_length, min_length=min_length, check_done_every=check_done_every,
                  compact_min=compact_min, repetition_penalty=float(repetition_penalty))
        if streams <= 1 or trace is not None or B < 2 * streams:
            g = self._beam_search(enc16, B, trace=trace, slot=0, **kw)
            while True:
                out = _advance(g)
                if out is not None:
                    return out
        main = torch.cuda.current_stream()
        side = self.__dict__.setdefault("_decode_streams", {})
        Te = enc16.shape[0] // B
        bounds = [(B * i // streams, B * (i + 1) // streams) for i in range(streams)]
        fork = torch.cuda.Event()
        fork.record(main)
        gens = []
        for i, (lo, hi) in enumerate(bounds):
            st = side.get((i, enc16.device))
            if st is None:
                st = side[(i, enc16.device)] = torch.cuda.Stream(device=enc16.device)
            st.wait_event(fork)
            gens.append((st, self._beam_search(enc16[lo * Te:hi * Te], hi - lo, slot=i, **kw)))
        results = [None] * streams
        live = list(range(streams))
        while live:
            for i in list(live):
                st, g = gens[i]
                with torch.cuda.stream(st):
                    results[i] = _advance(g)
                if results[i] is not None:
                    live.remove(i)
        for i, (st, _) in enumerate(gens):
            join = torch.cuda.Event()
            join.record(st)
            main.wait_event(join)
            for t in results[i]:
                t.record_stream(main)
        return torch.cat([r[0] for r in results]), torch.cat([r[1] for r in results])

    def _beam_search(self, enc16, B, **kw):
        """Generator: queues the prompt pass and one decode step per ``next()`` on the current stream, returns
        (tokens, lens) through StopIteration.  ``kw``: the keyword arguments of BeamSearch."""
        s = BeamSearch(self, enc16, B, **kw)
        # ---- prompt pass, once per image: the beams of an image are identical until the first update
        s.select(s.sess.prefill(s.prompt.contiguous().view(-1), s.P, shared=True), s.P, beams_in_logits=1)
        yield
        c = s.P + 1
        while c < s.max_length and not s.poll(c):
            if not s.run_step(c):
                return (yield from self._beam_search(enc16, B, **kw))    # (graphs are off now: the same search, plain launches)
            c += 1
            yield
        return s.finish(c)
