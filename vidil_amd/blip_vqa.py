"""BLIP question answering on the HIP kernels — drop-in for the reference's ``models/blip_vqa.py`` at inference:
``blip_vqa(pretrained, image_size, vit)``, ``BLIP_VQA.forward(image, question, answer=None, n=None, weights=None, train=True,
inference='rank', k_test=128)``.

Both inference modes start alike (models/blip_vqa.py:39-44,85-89): the ViT, the questions tokenised with padding='longest' at
most 35 tokens long with [ENC] first, and the image-grounded text encoder (``BertModel.encode``, question padding masked in its
self-attention).  The hidden states of ALL positions, pad positions included, are kept as 16-bit rows [Q*Tq, C]: they are the
encoder states of the answer decoder.

  * ``inference='generate'`` (:91-111): beam search (3 beams, at most 10 tokens, a one-token [DEC] prompt) over all Tq question
    states WITHOUT a mask — the reference hands ``generate`` an all-ones ``question_atts``, so the states of pad positions are
    attended.  The quirk is kept: a generated answer depends on the longest question of the call, as in the reference.
  * ``inference='rank'`` (:113-167): stage 1 takes the log-probability of every candidate's first token after [DEC]
    (``BertLMHeadModel.start_logits`` -> ``kernels.candidate_logprobs``, one read of the logits) and the ``k_test`` best per
    question (``kernels.topk_rows``); stage 2 scores those answers teacher-forced (``BertLMHeadModel.score``, label smoothing
    0.1 as ``-output.loss`` has it) and picks the best.  Cross-attention is masked to each question's real length in both.
    Two documented deviations: among EQUAL first-token probabilities the order is value descending, index ascending
    (``torch.topk`` leaves it unspecified), and ``k_test`` above the number of answers raises ``ValueError``.
  * ``train=True`` (:46-81) returns the value of the forward loss (no backward pass).

Plain f16 / bf16 operands only: the parity precision mode and fp8 are refused.  So are more than 768 image tokens per image
(what the attention kernels serve): the reference's default image_size=480 constructs and loads, its forward pass raises; use 384.

``BLIP_Video_VQA`` / ``blip_vqa_video()`` (models/blip_vqa.py:169-346) answer questions about a VIDEO: the ViT tokens of its N
frames are one encoder sequence of N*T keys (``video_embeds.view(B, -1, C)``, :201) — 8 x 197 = 1,576 at 224^2 —, at most
MAX_VIDEO_TOKENS, through the long-key form of ``vidil_attention``.  Its text encoder runs image-major (``group_start``): the
questions are sorted by video, a video's cross-attention K / V are projected once whatever the number of its questions, and
one staging of them serves every question of the video (``question_states_grouped``).  Everything behind the
question states — ``rank_answer``, ``generate_answer_ids``, ``answer_loss`` — is BLIP_VQA's.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import kernels as K
from . import video as V
from .blip import create_vit, load_checkpoint, resolve_med_config
from .decoding import BeamSearchMixin
from .med import BertConfig, BertLMHeadModel, BertModel
from .packing import FP8, compute_dtype, fp8_companion, require_cuda, set_compute_dtype, set_parity_mode
from .tokenizer import init_tokenizer, refuse_synthetic_with_checkpoint
from .video import MAX_VIDEO_TOKENS  # noqa: F401  (its home is video.py; imported from here too)

VQA_QUESTION_MAX_LENGTH = 35     # models/blip_vqa.py:42
VQA_NUM_BEAMS, VQA_MAX_LENGTH, VQA_MIN_LENGTH = 3, 10, 1    # models/blip_vqa.py:92,100-102
VQA_LABEL_SMOOTHING = 0.1        # models/med.py:916 (the loss `rank_answer` negates)
MAX_IMAGE_TOKENS = 768           # keys the attention kernels serve (vidil_attention: Nk <= 768): ViT-B/16 up to 432 px


class BLIP_VQA(BeamSearchMixin, nn.Module):
    #: read by packing.set_parity_mode / set_compute_dtype: why this model refuses the parity precision mode and fp8
    plain_only = "question answering is built for plain f16 / bf16 operands (masked cross-attention has no error-compensated form)"

    def __init__(self, med_config="configs/med_config.json", image_size=480, vit="base", vit_grad_ckpt=False, vit_ckpt_layer=0,
                 tokenizer=None):
        super().__init__()
        self.visual_encoder, vision_width = create_vit(vit, image_size, vit_grad_ckpt, vit_ckpt_layer, drop_path_rate=0.1)
        self.tokenizer = tokenizer if tokenizer is not None else init_tokenizer()
        encoder_config = BertConfig.from_json_file(resolve_med_config(med_config))
        encoder_config.encoder_width = vision_width
        self.text_encoder = BertModel(config=encoder_config, add_pooling_layer=False)
        decoder_config = BertConfig.from_json_file(resolve_med_config(med_config))
        if decoder_config.encoder_width != decoder_config.hidden_size:
            raise ValueError(f"BLIP_VQA: the answer decoder attends to the text encoder's states, so med_config's encoder_width "
                             f"({decoder_config.encoder_width}) must equal hidden_size ({decoder_config.hidden_size})")
        self.text_decoder = BertLMHeadModel(config=decoder_config)
        # pinned to plain 16-bit operands, so that the process-wide $VIDIL_PARITY / $VIDIL_DTYPE=fp8 defaults — meant for the
        # captioner, the filter and CLIP — leave a fresh model as it is (as BLIP_Retrieval does)
        set_parity_mode(False, self)
        if compute_dtype(self) == FP8:
            set_compute_dtype(fp8_companion(), self)

    # ------------------------------------------------------------------ precision
    def _require_plain(self):
        V.require_plain(self, "BLIP_VQA", "question answering", "masked cross-attention has no error-compensated form")

    def _require_image_tokens(self, n_tokens=None):
        """The ViT's self-attention and the text encoder's cross-attention run over all image tokens, and the attention
        kernels serve at most MAX_IMAGE_TOKENS keys: refuse more here, by name, before anything is launched."""
        if n_tokens is None:
            n_tokens = self.visual_encoder.patch_embed.num_patches + 1
        if n_tokens > MAX_IMAGE_TOKENS:
            raise ValueError(f"BLIP_VQA: {n_tokens} image tokens per image exceed the {MAX_IMAGE_TOKENS} keys the attention kernels "
                             f"serve (ViT-B/16: image_size <= 432; the reference's default 480 gives 901) — build the model with "
                             f"image_size=384, checkpoints' position embeddings are interpolated on load")

    # ------------------------------------------------------------------ tokenisation
    def tokenize_questions(self, question):
        """models/blip_vqa.py:42-44: padding='longest', truncation at 35 tokens, first id := [ENC].
        Returns (ids i32 [Q, Tq], lens i32 [Q]) on the host."""
        enc = self.tokenizer(list(question), padding="longest", truncation=True, max_length=VQA_QUESTION_MAX_LENGTH,
                             return_tensors="pt")
        ids = enc.input_ids.clone()
        ids[:, 0] = self.tokenizer.enc_token_id
        return ids.to(torch.int32), enc.attention_mask.sum(dim=1).to(torch.int32)

    def tokenize_answers(self, answer):
        """models/blip_vqa.py:51-52: padding='longest', first id := [DEC]; or an object that already holds ``input_ids`` /
        ``attention_mask`` in that form (what the reference's evaluation loop passes).  Returns (ids int64 [A, Ta], lens int64
        [A]) on the host."""
        if hasattr(answer, "input_ids") and hasattr(answer, "attention_mask"):
            return (torch.as_tensor(answer.input_ids).cpu().long().clone(),
                    torch.as_tensor(answer.attention_mask).cpu().long().sum(dim=1))
        enc = self.tokenizer(list(answer), padding="longest", return_tensors="pt")
        ids = enc.input_ids.clone().long()
        ids[:, 0] = self.tokenizer.bos_token_id
        return ids, enc.attention_mask.sum(dim=1).long()

    # ------------------------------------------------------------------ question states
    @torch.no_grad()
    def question_states(self, enc16, Q, ids, lens):
        """models/blip_vqa.py:85-89: image tokens enc16 [Q*Te, width] (one image per question) and question ids i32 [Q, Tq] /
        lens i32 [Q] -> (h32, h16) [Q*Tq, C], every position's last hidden state (pad positions too)."""
        require_cuda(enc16, "BLIP_VQA")
        self._require_plain()
        dev = enc16.device
        Te = enc16.shape[0] // Q
        self._require_image_tokens(Te)
        cross = self.text_encoder.project_cross_kv(enc16, Q, Te)
        return self.text_encoder.encode(ids.to(dev).contiguous(), lens.to(dev).to(torch.int32).contiguous(), cross)

    # ------------------------------------------------------------------ generate
    def prompt_ids(self, B, device):
        """models/blip_vqa.py:97: the one-token [DEC] prompt."""
        return torch.full((B, 1), self.tokenizer.bos_token_id, dtype=torch.int32, device=device)

    @torch.no_grad()
    def generate_answer_ids(self, states16, Q):
        """The captioner's beam search (BeamSearchMixin.generate_ids) over the UNMASKED question states [Q*Tq, C] (see the
        module docstring).  Returns (tokens i32 [Q, 10]: [DEC], the answer, [SEP] if it fits, then [PAD]; lens i32 [Q])."""
        self._require_plain()
        return self.generate_ids(states16, Q, num_beams=VQA_NUM_BEAMS, max_length=VQA_MAX_LENGTH, min_length=VQA_MIN_LENGTH)

    # ------------------------------------------------------------------ rank
    @torch.no_grad()
    def first_token_logprobs(self, states16, Q, q_lens, answer_ids):
        """Stage 1 of rank_answer (models/blip_vqa.py:123-135): f32 [Q, A] log-probability of every answer's first token after
        [DEC], cross-attention masked to each question's length.  Orders exactly as the reference's softmax probabilities."""
        dev = states16.device
        logits = self.text_decoder.start_logits(states16, Q, int(answer_ids[0, 0]), cross_kv_len=q_lens)
        first = answer_ids[:, 1].to(torch.int32).to(dev).contiguous()
        return K.candidate_logprobs(logits, first)

    @torch.no_grad()
    def rank_answer(self, states16, Q, q_lens, answer_ids, answer_lens, k):
        """models/blip_vqa.py:120-167.  states16 [Q*Tq, C], q_lens int [Q], answer_ids int64 [A, Ta] ([DEC] first, right-padded),
        answer_lens int64 [A] (host).  Returns (max_ids int64 [Q] device, topk_ids i32 [Q, k] device, log_probs_sum f32 [Q, k]
        device)."""
        self._require_plain()
        A = answer_ids.shape[0]
        if k > A:
            raise ValueError(f"BLIP_VQA rank: k_test={k} exceeds the number of answers ({A})")
        if k < 1 or answer_ids.shape[1] < 2:
            raise ValueError("BLIP_VQA rank: k_test >= 1 and answers of at least one token behind [DEC] expected")
        lp = self.first_token_logprobs(states16, Q, q_lens, answer_ids)
        _, topk_ids = K.topk_rows(lp, k)                       # (value descending, index ascending; k <= 128, A <= 38,400)
        pick = topk_ids.cpu().long().view(-1)
        if bool((pick < 0).any()):                             # (topk_rows: -1 where a row has fewer than k values above -inf)
            raise ValueError(f"BLIP_VQA rank: a question has fewer than k_test={k} answers whose first token has a finite log-probability")
        res = self.text_decoder.score(states16, Q, answer_ids[pick], answer_lens[pick],
                                      image_index=torch.arange(Q).repeat_interleave(k), label_smoothing=VQA_LABEL_SMOOTHING,
                                      prompt_length=1, cross_kv_len=q_lens)
        log_probs_sum = (-res.loss_sum).view(Q, k)
        max_topk_ids = log_probs_sum.argmax(dim=1)
        max_ids = topk_ids.long().gather(1, max_topk_ids[:, None])[:, 0]
        return max_ids, topk_ids, log_probs_sum

    # ------------------------------------------------------------------ loss
    @torch.no_grad()
    def answer_loss(self, states16, Q, q_lens, answer_ids, answer_lens, n):
        """models/blip_vqa.py:61-76: question b owns the next n[b] answers; the label-smoothed loss summed per answer, f32 [sum n]."""
        n = torch.as_tensor(n).cpu().long().view(-1)
        if n.numel() != Q or int(n.sum()) != answer_ids.shape[0]:
            raise ValueError(f"BLIP_VQA: n must hold {Q} counts that sum to the {answer_ids.shape[0]} answers")
        res = self.text_decoder.score(states16, Q, answer_ids, answer_lens, image_index=torch.arange(Q).repeat_interleave(n),
                                      label_smoothing=VQA_LABEL_SMOOTHING, prompt_length=1, cross_kv_len=q_lens)
        return res.loss_sum

    def _answer(self, states16, Q, lens, answer, n, weights, train, inference, k_test):
        """What ``forward`` does behind the question states (models/blip_vqa.py:46-116; BLIP_Video_VQA: :208-280)."""
        if train:
            a_ids, a_lens = self.tokenize_answers(answer)
            loss = self.answer_loss(states16, Q, lens, a_ids, a_lens, n)
            w = torch.as_tensor(weights, dtype=torch.float32).to(loss.device).view(-1)
            return ((w.double() * loss.double()).sum() / Q).float()
        if inference == "generate":
            out_tok, _ = self.generate_answer_ids(states16, Q)
            return [self.tokenizer.decode(row, skip_special_tokens=True) for row in out_tok.cpu().tolist()]
        a_ids, a_lens = self.tokenize_answers(answer)
        return self.rank_answer(states16, Q, lens, a_ids, a_lens, k_test)[0]

    @torch.no_grad()
    def forward(self, image, question, answer=None, n=None, weights=None, train=True, inference="rank", k_test=128):
        """Reference: models/blip_vqa.py:37-116.  image f32 [Q,3,S,S] on the GPU, one per question.
        train=True: the 0-dim f32 loss (weights * per-answer loss).sum() / Q, no backward pass; train=False, 'generate':
        list[str]; train=False, 'rank': int64 [Q] indices into the answer list, on the GPU."""
        self._require_image_tokens()
        require_cuda(image, "BLIP_VQA.forward")
        self._require_plain()
        if not train and inference not in ("generate", "rank"):
            raise ValueError(f"unknown inference {inference!r} (generate | rank)")
        if not train and inference == "generate":
            K.require_num_beams(VQA_NUM_BEAMS, "BLIP_VQA generate")          # (before the ViT runs)
        Q = image.shape[0]
        _, y16 = self.visual_encoder.forward_both(image)
        ids, lens = self.tokenize_questions(question)
        if ids.shape[0] != Q:
            raise ValueError(f"BLIP_VQA: {ids.shape[0]} questions for {Q} images")
        _, states16 = self.question_states(y16, Q, ids, lens)
        return self._answer(states16, Q, lens, answer, n, weights, train, inference, k_test)


def blip_vqa(pretrained="", **kwargs):
    """Reference: models/blip_vqa.py:334-339 (does not assert on the missing keys)."""
    model = BLIP_VQA(**kwargs)
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
    return model


# ====================================================================================================== video
def video_major_order(video_of_question, n_videos):
    """The video-major order of questions that arrive in any order (host index tensors; pure).

    video_of_question int [Q]: the video every question asks about.  Returns a dict: ``order`` int64 [Q] — the caller's index of
    the question at every sorted position (stable: a video's questions keep the caller's order); ``inverse`` int64 [Q] — the
    sorted position of every caller's question (``sorted[inverse]`` is the caller's order again); ``group_start`` int32
    [n_videos+1] — the sorted questions of video v are group_start[v] .. group_start[v+1]-1 (empty for a video nobody asks
    about); ``max_group`` — its largest gap."""
    v = torch.as_tensor(video_of_question).cpu().long().view(-1)
    group_start, max_group = V.group_table(v, n_videos, "video_of_question")
    order = torch.argsort(v, stable=True)
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(v.numel())
    return dict(order=order, inverse=inverse, group_start=group_start, max_group=max_group)


class BLIP_Video_VQA(BLIP_VQA):
    """models/blip_vqa.py:169-331: BLIP_VQA over ``video_representation: concat_frame``.  Same members and parameter names, so
    a BLIP_VQA checkpoint loads as it does there."""

    def _require_video_tokens(self, n_tokens):
        V.require_video_tokens(n_tokens, "BLIP_Video_VQA")

    # ------------------------------------------------------------------ frames -> tokens
    def video_tokens(self, video):
        """f32 [B,N,3,S,S] (normalised) -> 16-bit [B*N*T, width]: one ViT pass (video.frame_tokens; models/blip_vqa.py:198-201)."""
        self._require_image_tokens()
        self._require_plain()
        return V.frame_tokens(self.visual_encoder, video, who="BLIP_Video_VQA.video_tokens", u8=False)

    def video_tokens_u8(self, frames_u8):
        """uint8 [B,N,S,S,3] frames (already S x S) -> the same, with /255 and the normalisation fused into the patch kernel."""
        self._require_image_tokens()
        self._require_plain()
        return V.frame_tokens(self.visual_encoder, frames_u8, who="BLIP_Video_VQA.video_tokens_u8", u8=True)

    # ------------------------------------------------------------------ question states, a video shared by its questions
    @torch.no_grad()
    def question_states_grouped(self, tokens16, B, ids, lens, video_of_question, videos_per_block=None, timings=None, f32=True):
        """models/blip_vqa.py:217-221,248-252 for Q questions about B videos, in ANY order.  tokens16 16-bit [B*Te, width] (Te =
        N*T tokens per video, or T of one frame); ids i32 [Q, Tq] / lens i32 [Q] (``tokenize_questions``); video_of_question
        int [Q].  Returns (h32, h16) [Q*Tq, C] in the caller's order: every position's last hidden state (pad positions too).

        The questions are sorted video-major (``video_major_order``) and the videos walked in blocks of ``videos_per_block``
        (default: what fits video.KV_BLOCK_BYTES): a block's cross-attention K / V are projected ONCE per video and
        the text encoder runs over the block's questions with the ``group_start`` table, so one staging of a video's K / V
        serves all its questions; a video without a question is an empty group.  Every block is launched with the same Tq
        (ids' width: the longest question of the call) and the same ``max_group`` bound — the largest group of the call,
        rounded up to more than 32 query rows per video, which the kernels past 768 keys need and which keeps one kernel
        family (row-major values) at every group size: row tiles past a video's last question return at once.  A question's
        bits therefore do not depend on the block size.
        ``f32=False``: the f32 copy of the states is not assembled and None is returned in its place (the answer decoder reads
        the 16-bit rows only).  The blocks' rows are joined by one copy (none when the call is one block) and put into the
        caller's order by one ``index_select`` (none when the questions arrive video-major).
        ``timings`` (dict, optional): receives the seconds spent in ``kv`` / ``encoder`` (video.phase_timer)."""
        require_cuda(tokens16, "BLIP_Video_VQA")
        self._require_plain()
        Te = V.video_rows(tokens16, B, "BLIP_Video_VQA")
        Q, Tq = ids.shape
        sched = video_major_order(video_of_question, B)
        if sched["order"].numel() != Q or lens.numel() != Q:
            raise ValueError(f"BLIP_Video_VQA: {Q} questions, {lens.numel()} lengths and {sched['order'].numel()} entries of "
                             f"video_of_question")
        te, dev = self.text_encoder, tokens16.device
        C = te.config.hidden_size
        order = sched["order"]
        max_group = max(sched["max_group"], -(-33 // Tq))
        ids_s = ids.cpu()[order].to(torch.int32).to(dev).contiguous()
        lens_s = lens.cpu()[order].to(torch.int32).to(dev).contiguous()
        parts32, parts16 = [], []
        if videos_per_block is None:
            videos_per_block = V.videos_per_block(te.config, Te)
        if videos_per_block < 1:
            raise ValueError(f"BLIP_Video_VQA: videos_per_block={videos_per_block}")
        lap = V.phase_timer(timings)
        for b0, b1, p0, p1, groups in V.blocks(sched["group_start"], B, videos_per_block):
            t0 = lap()
            cross = te.project_cross_kv(tokens16[b0 * Te:b1 * Te], b1 - b0, Te, v_rowmajor=True)
            t0 = lap("kv", t0)
            a32, a16 = te.encode(ids_s[p0:p1], lens_s[p0:p1], cross, cross_groups=groups.to(dev).contiguous(), cross_max_group=max_group)
            if f32:
                parts32.append(a32)
            parts16.append(a16)
            lap("encoder", t0)
        back = None if torch.equal(order, torch.arange(Q)) else sched["inverse"].to(dev)

        def joined(parts):                   # (blocks are in sorted order and every question belongs to one of them)
            h = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
            return h if back is None else h.view(Q, Tq, C).index_select(0, back).view(Q * Tq, C)

        return (joined(parts32) if f32 else None), joined(parts16)

    # ------------------------------------------------------------------ the reference's call
    @torch.no_grad()
    def forward(self, video, question, answer=None, n=None, weights=None, train=True, inference="rank", k_test=128):
        """Reference: models/blip_vqa.py:196-280.  video f32 [B,N,3,S,S] on the GPU, one question per video.
        train=True: the 0-dim f32 loss (weights * per-answer loss).sum() / B, no backward pass; train=False, 'generate':
        list[str]; train=False, 'rank': int64 [B] indices into the answer list, on the GPU.  The case video_of_question =
        arange(B) of ``question_states_grouped``."""
        if not train and inference not in ("generate", "rank"):
            raise ValueError(f"unknown inference {inference!r} (generate | rank)")
        if not train and inference == "generate":
            K.require_num_beams(VQA_NUM_BEAMS, "BLIP_Video_VQA generate")    # (before the ViT runs)
        B = video.shape[0]
        ids, lens = self.tokenize_questions(question)
        if ids.shape[0] != B:
            raise ValueError(f"BLIP_Video_VQA: {ids.shape[0]} questions for {B} videos")
        tokens = self.video_tokens(video)
        _, states16 = self.question_states_grouped(tokens, B, ids, lens, torch.arange(B))
        return self._answer(states16, B, lens, answer, n, weights, train, inference, k_test)


def blip_vqa_video(pretrained="", **kwargs):
    """Reference: models/blip_vqa.py:341-346 (does not assert on the missing keys)."""
    model = BLIP_Video_VQA(**kwargs)
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
    return model
