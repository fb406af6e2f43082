"""Fractional pod side of the pod server (server.py): stdlib + numpy only.

A pod scheduled onto a pod-server slice gets, from the device plugin,
``NOS_AMD_POD_SERVER`` (its GPU's server socket, in the one per-GPU directory
the container mounts), ``NOS_AMD_POD_TOKEN`` (the allocation's token: the
server reads the slice's memory and CU mask from the plugin's record of it),
``NOS_AMD_MEMORY_LIMIT_GB`` (informational) and no ``/dev/kfd`` or render
node.  The container never opens the GPU.  It registers its model once -- a
program (op graph + weights, program.py) -- then sends inference requests.
This is the role MPS clients play in the reference: their CUDA calls go to
the MPS server, which runs them in the server's context.

Server loss.  A request whose connection breaks raises
:class:`PodServerGone` (the pod exits non-zero and the kubelet restarts it),
unless the client was made with ``reconnect_s`` > 0: it then waits up to that
long for the server (the supervisor restarts a dead one), registers the same
program again with the same token, and retries the request once.
"""
from __future__ import annotations

import os
import socket
import time

import numpy as np

from ..api.constants import ENV_MEMORY_LIMIT_GB, ENV_POD_CU_MASK, ENV_POD_SERVER, ENV_POD_TOKEN
from . import protocol as P


_GREEDY = {"temperature": 0.0, "top_k": 0, "top_p": 1.0, "seed": 0}   # the sampling defaults: not sent


class PodServerError(RuntimeError):
    pass


class PodServerGone(PodServerError):
    """The connection to the pod server broke (server died or evicted us)."""


def _connect(path: str, timeout_s: float) -> socket.socket:
    deadline = time.monotonic() + timeout_s
    while True:  # the server's socket appears once it accepts (server.start)
        s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        try:
            s.connect(path)
            return s
        except (FileNotFoundError, ConnectionRefusedError):
            s.close()
            if time.monotonic() > deadline:
                raise PodServerError(f"no pod server at {path} after {timeout_s} s")
            time.sleep(0.1)


def _adapter_field(adapter) -> int | list:
    """A request's ``"adapter"``: an int (every row) or a list of ints (the server checks the values)."""
    if isinstance(adapter, (int, np.integer)) and not isinstance(adapter, bool):
        return int(adapter)
    return [int(a) if isinstance(a, np.integer) else a for a in adapter]


def _wire(a, want: str | None, what: str) -> np.ndarray:
    """``a`` as the bytes the tenant reads: the registered program's type
    (``want``, from the register reply) decides, not the array's -- a uint8
    image or an int arange for an fp32 model goes as float32 values.  Float
    data for an id input is refused rather than truncated.  Without ``want``
    (no register reply seen) integer arrays go as int32, others as float32."""
    a = np.asarray(a)
    is_int = np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_
    if want == "i32":
        if not is_int:
            raise PodServerError(f"{what}: the tenant's model takes integer ids, got {a.dtype}")
        return np.ascontiguousarray(a, dtype=np.int32)
    if want == "f32" or not is_int:
        return np.ascontiguousarray(a, dtype=np.float32)
    return np.ascontiguousarray(a, dtype=np.int32)


class PodClient:
    def __init__(self, path: str | os.PathLike, connect_timeout_s: float = 60.0, reconnect_s: float = 0.0):
        self.path = str(path)
        self.sock = _connect(self.path, connect_timeout_s)
        self.reconnect_s = reconnect_s
        self.tenant: int | None = None
        self.info: dict = {}
        self._reg: tuple[dict, bytes] | None = None
        self.input_dtype: str | None = None    # "f32" / "i32": the registered program's input (register reply)
        self.target_dtype: str | None = None   # a training tenant's target
        self.reconnects = 0

    @classmethod
    def from_env(cls, env: dict | None = None, **kw) -> "PodClient":
        env = os.environ if env is None else env
        path = env.get(ENV_POD_SERVER)
        if not path:
            raise PodServerError(f"{ENV_POD_SERVER} is not set: this pod was not allocated a pod-server slice")
        return cls(path, **kw)

    def _call(self, req: dict, payload: bytes = b"", reply_limit: int | None = None) -> tuple[dict, bytes]:
        if self.sock is None:
            raise PodServerGone("client is closed")
        try:
            P.send_msg(self.sock, req, payload)
            rep, data = P.recv_msg(self.sock, None if reply_limit is None else (lambda obj, n: reply_limit))
        except (ConnectionError, OSError) as e:
            raise PodServerGone(f"pod server connection lost: {e}") from e
        if not rep.get("ok"):
            raise PodServerError(rep.get("error", "pod server error"))
        return rep, data

    def register(self, pod: str, program: dict, weights: bytes = b"", token: str | None = None,
                 memory_limit_gb: float | None = None, cu_mask: str | None = None, env: dict | None = None,
                 variants: list[dict] | None = None, train: dict | None = None,
                 priority: str | None = None) -> dict:
        """Ship the pod's program (op graph + weight bytes, program.py) to the
        server.  The allocation token comes from the device plugin's env; the
        slice itself is the plugin's record.  ``memory_limit_gb`` /
        ``cu_mask`` matter only to a server without allocation records.
        ``variants``: the same model's programs for other input shapes (over
        the same ``weights``); :meth:`infer` routes by the input's shape.
        ``train``: register a training tenant (podserver/training.py: loss,
        optimizer, lr, ...) driven by :meth:`train_step`."""
        env = os.environ if env is None else env
        if memory_limit_gb is None and env.get(ENV_MEMORY_LIMIT_GB):
            memory_limit_gb = float(env[ENV_MEMORY_LIMIT_GB])
        req = {"op": "register", "pod": pod, "program": program, "token": token or env.get(ENV_POD_TOKEN),
               "memory_limit_gb": memory_limit_gb, "cu_mask": cu_mask or env.get(ENV_POD_CU_MASK)}
        if variants:
            req["variants"] = list(variants)
        if train is not None:
            req["train"] = dict(train)
        if priority is not None:   # "latency": the server's priority lanes (default for stateful programs)
            req["priority"] = priority
        rep, _ = self._call(req, weights)
        self._reg = (req, weights)
        self.input_dtype = rep.get("input_dtype")
        self.target_dtype = rep.get("target_dtype")
        self.tenant = rep["tenant"]
        self.info = rep
        return rep

    def _reregister(self) -> None:
        deadline = time.monotonic() + self.reconnect_s
        last = None
        while time.monotonic() < deadline:
            try:
                self.sock.close()
            except OSError:
                pass
            try:
                self.sock = _connect(self.path, max(0.1, deadline - time.monotonic()))
                rep, _ = self._call(*self._reg)
                self.tenant, self.info = rep["tenant"], rep
                self.reconnects += 1
                return
            except PodServerError as e:  # not up yet / still holding our old tenant: retry
                last = e
                time.sleep(0.2)
        raise PodServerGone(f"pod server did not come back within {self.reconnect_s} s: {last}")

    def infer(self, x: np.ndarray | None = None, outputs: bool | list = False,
              sampling: dict | None = None, stopping: dict | None = None,
              adapter: int | list | None = None) -> tuple[list[np.ndarray], dict]:
        """One inference on the pod's model; ``x`` replaces the resident input
        (one of the registered input shapes; without ``x`` the primary
        shape's resident input runs).  ``outputs``: return every output
        (True), none, or those of the listed indices.  A stateful tenant's
        reply carries its counters (``rep["state"]``, e.g. the position).
        ``sampling``: ``{"temperature", "top_k", "top_p", "seed"}`` (any
        subset) for a tenant whose programs end in ``sample``; without it the
        request is greedy.  ``stopping``: ``{"stop_ids", "pad_id",
        "repetition_penalty"}`` (any subset) for a tenant registered with
        stopping programs; the reply's ``state`` then carries the rows'
        ``done`` flags beside ``pos``.  ``adapter``, for a tenant registered with
        LoRA adapters (``llama_decode_programs(..., adapters=[...])``): the
        adapter of every row (an int) or of each row (a list), 1 .. N, 0 or
        nothing: the base model."""
        req = {"op": "infer", "outputs": outputs}
        if adapter is not None:
            req["adapter"] = _adapter_field(adapter)
        if sampling:
            req["sampling"] = dict(sampling)
        if stopping:
            req["stopping"] = dict(stopping)
        if x is None:
            payload = b""
        else:
            wire = _wire(x, self.input_dtype, "input")
            payload = wire.tobytes()
            req["shape"] = [int(d) for d in np.shape(x)]
            req["dtype"] = "i32" if wire.dtype == np.int32 else "f32"
        try:
            rep, data = self._call(req, payload)
        except PodServerGone:
            if self.reconnect_s <= 0 or self._reg is None:
                raise
            self._reregister()
            rep, data = self._call(req, payload)
        return (P.unpack_arrays(rep["outputs"], data) if outputs else []), rep

    def reset(self) -> dict:
        """Zero a stateful tenant's state (K / V caches, positions): a new
        sequence.  Returns the reply (``state``: the counters, now 0)."""
        return self._call({"op": "reset"})[0]

    def generate(self, prompt: np.ndarray, max_new_tokens: int, next_output: int = -1,
                 server_loop: bool = True, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                 seed: int = 0, eos_token_id: int | list | None = None, pad_token_id: int | None = None,
                 repetition_penalty: float = 1.0, speculate: bool = False,
                 prefill_len: int | None = None, adapter: int | list | None = None) -> tuple[np.ndarray, dict]:
        """Generation on a stateful decoder tenant
        (models/llama_program.llama_decode_programs): the prompt ids [B, P]
        go to the prefill variant, then the decode variant runs once per new
        token, fed the program's next-ids output (``next_output``).
        ``server_loop``: the decode steps run as ONE ``generate`` request --
        the server replays the decode graph back to back, feeding the ids on
        the device, and returns every token at the end (no host round trip
        per token); otherwise one [B, 1] request per token.  ``temperature``
        (0: greedy), ``top_k`` (0: off), ``top_p`` (1: off) and ``seed`` go
        with every request of the generation when they differ from these
        defaults, for a tenant registered with sampling programs
        (``llama_decode_programs(..., sampling=True)``): the ids are then
        drawn on the device, the same ones on either path and on every
        repeat of the sequence with the same seed.

        ``eos_token_id`` (an int or a list of at most four), ``pad_token_id``
        (default: the first stop id) and ``repetition_penalty``, for a tenant
        registered with stopping programs (``llama_decode_programs(...,
        stopping=True)``), are transformers' ``generate`` arguments of those
        names: a row ends with its first stop id and emits the pad id from
        then on, and the generation ends once every row has -- the server
        loop leaves its loop then, the per-request path stops sending.

        Returns (ids [B, n], timings): n = ``max_new_tokens``, or fewer with
        stop ids (what ``generate(...)[:, P:]`` of transformers returns; 1
        when the prefill draws every row's stop id); the prefill's round
        trip, every decode step's (server loop: the loop's time / steps),
        ``steps_run`` (the decode steps the server ran: with stop ids up to
        two check windows more than n - 1) and the server's final counters.

        ``speculate``, for a tenant registered with a verify program
        (``llama_decode_programs(..., speculate=K)``; greedy, no stop ids):
        the prefill, then ONE ``generate`` request over the verify variant
        (:meth:`speculate_loop`) -- the same ``max_new_tokens`` ids as the
        plain tenant's in fewer steps; the timings also carry ``n_acc``
        [steps_run, B], the positions each verify step advanced.
        ``prefill_len`` (with ``speculate``; default: the whole prompt): only
        the prompt's first that many ids go to the prefill variant, the rest
        one decode step each -- for a prompt as long as the verify step is
        wide, whose shape would name two variants.

        ``adapter`` (an int, or a list of one int per row), for a tenant
        registered with LoRA adapters: it goes with every request of the
        generation, on either path and with ``speculate``."""
        prompt = np.asarray(prompt)
        B = prompt.shape[0]
        lora = {} if adapter is None else {"adapter": _adapter_field(adapter)}
        if speculate:
            if temperature != 0.0 or top_k or top_p != 1.0 or eos_token_id is not None or repetition_penalty != 1.0:
                raise ValueError("generate: speculate is greedy only, without stop ids or a repetition penalty")
            t0 = time.monotonic()
            head = prompt.shape[1] if prefill_len is None else int(prefill_len)
            if not 0 < head <= prompt.shape[1]:
                raise ValueError(f"generate: prefill_len must lie in [1, {prompt.shape[1]}]")
            outs, rep = self.infer(prompt[:, :head], outputs=[1, 2], **lora)   # next_ids, spec_ids (the pending token, drafts)
            for s in range(head, prompt.shape[1]):   # the drafts after single steps: the pending token repeated
                o, rep = self.infer(prompt[:, s:s + 1], outputs=[1], **lora)
                outs = [o[0], np.repeat(o[0].reshape(B, 1), outs[1].reshape(B, -1).shape[1], axis=1)]
            t1 = time.monotonic()
            if max_new_tokens <= 1:
                return outs[0].reshape(B, 1).astype(np.int32), {"prefill_s": t1 - t0, "step_s": [], "steps_run": 0,
                                                                "state": rep.get("state"), "n_acc": np.zeros((0, B), np.int32)}
            s0 = time.monotonic()
            toks, acc, rep = self.speculate_loop(outs[1].reshape(B, -1).astype(np.int32), max_new_tokens - 1,
                                                 prompt.shape[1] + max_new_tokens - 1, adapter=adapter)
            dt = time.monotonic() - s0
            run = int(rep["steps_run"])
            return toks, {"prefill_s": t1 - t0, "step_s": [dt / run] * run, "state": rep.get("state"),
                          "steps_run": run, "n_acc": acc}
        given = {"temperature": temperature, "top_k": top_k, "top_p": top_p, "seed": seed}
        sampling = {k: v for k, v in given.items() if v != _GREEDY[k]}   # older servers keep serving greedy clients
        stops = [] if eos_token_id is None else ([eos_token_id] if isinstance(eos_token_id, (int, np.integer))
                                                 else list(eos_token_id))
        stopping = {}
        if stops:
            stopping["stop_ids"] = [int(v) if isinstance(v, np.integer) else v for v in stops]
        if pad_token_id is not None:
            stopping["pad_id"] = int(pad_token_id) if isinstance(pad_token_id, np.integer) else pad_token_id
        if repetition_penalty != 1.0:
            stopping["repetition_penalty"] = repetition_penalty
        extra = {**({"sampling": sampling} if sampling else {}), **({"stopping": stopping} if stopping else {}), **lora}

        def ended(rep) -> bool:
            done = (rep.get("state") or {}).get("done")
            return bool(stops) and done is not None and all(done)

        t0 = time.monotonic()
        outs, rep = self.infer(prompt, outputs=[next_output], **extra)
        t1 = time.monotonic()
        tok = outs[0].reshape(B, -1)[:, -1].astype(np.int32)
        toks, steps = [tok], []
        n = 0 if ended(rep) else max_new_tokens - 1
        run = 0
        if server_loop and n > 0:
            wire = _wire(tok.reshape(B, 1), self.input_dtype, "input")
            req = {"op": "generate", "steps": n, "output": next_output, "shape": [B, 1],
                   "dtype": "i32" if wire.dtype == np.int32 else "f32", **extra}
            s0 = time.monotonic()
            rep, data = self._call(req, wire.tobytes())
            dt = time.monotonic() - s0
            out = P.unpack_arrays(rep["outputs"], data)[0]
            ids = out.reshape(out.shape[0], B, -1)[:, :, -1].astype(np.int32)
            toks += list(ids)
            run = int(rep.get("steps_run", n))
            steps = [dt / run] * len(ids)
        else:
            for _ in range(n):
                s0 = time.monotonic()
                outs, rep = self.infer(tok.reshape(B, 1), outputs=[next_output], **extra)
                steps.append(time.monotonic() - s0)
                tok = outs[0].reshape(B, -1)[:, -1].astype(np.int32)
                toks.append(tok)
                run += 1
                if ended(rep):
                    break
        return np.stack(toks, axis=1), {"prefill_s": t1 - t0, "step_s": steps, "state": rep.get("state"),
                                        "steps_run": run}

    def speculate_loop(self, ids: np.ndarray, steps: int, end: int,
                       adapter: int | list | None = None) -> tuple[np.ndarray, np.ndarray, dict]:
        """A speculating tenant's verify loop as ONE ``generate`` request.
        ``ids`` [B, K]: the pending token of each row (the last id drawn, at
        position ``pos``) and K - 1 drafts (any valid ids; a prefill's
        ``spec_ids``, or the pending token repeated after single decode
        steps).  The server replays the verify variant, feeding its
        ``next_ids``, until every row's counter is at ``end`` -- ``steps`` =
        ``end - pos`` runs at the most.  Returns (the tokens at positions
        ``end - steps .. end`` [B, steps + 1], the pending one first; each
        step's advance ``n_acc`` [steps_run, B]; the reply, with
        ``steps_run`` and the final counters)."""
        ids = np.asarray(ids)
        B = ids.shape[0]
        wire = _wire(ids, self.input_dtype, "input")
        req = {"op": "generate", "steps": int(steps), "output": 1, "shape": [int(d) for d in ids.shape],
               "dtype": "i32" if wire.dtype == np.int32 else "f32", "speculate": {"end": int(end)}}
        if adapter is not None:
            req["adapter"] = _adapter_field(adapter)
        rep, data = self._call(req, wire.tobytes())
        toks, acc = P.unpack_arrays(rep["outputs"], data)
        return toks.reshape(B, -1).astype(np.int32), acc.reshape(-1, B).astype(np.int32), rep

    def train_step(self, x: np.ndarray, target: np.ndarray) -> dict:
        """One optimisation step of a training tenant on (x, target): the
        target has the trained output's shape (mse, float) or its shape
        without the class dim (cross_entropy, int class ids).  Returns the
        reply: ``loss`` (before the step's update), ``step``, timings."""
        xa = _wire(x, self.input_dtype, "input")
        ta = _wire(target, self.target_dtype, "target")
        xb = xa.tobytes()
        return self._call({"op": "train", "x_bytes": len(xb), "dtype": "i32" if xa.dtype == np.int32 else "f32",
                           "target_dtype": "i32" if ta.dtype == np.int32 else "f32"}, xb + ta.tobytes())[0]

    def weights(self) -> bytes:
        """A training tenant's current weights in its program's payload
        layout: ``register(program, weights=...)`` resumes from them."""
        # a weight payload may exceed the protocol's default 1 GiB reply bound
        # (the server's slice bounds it); the caller asked for all of it
        return self._call({"op": "weights"}, reply_limit=1 << 42)[1]

    def checkpoint(self) -> bytes:
        """A training tenant's weights followed by its optimizer state:
        ``register(program, weights=<this>, train={..., "resume": True})``
        continues the run where it stopped."""
        return self._call({"op": "checkpoint"}, reply_limit=1 << 42)[1]

    def stats(self) -> dict:
        return self._call({"op": "stats"})[0]

    def close(self) -> None:
        if self.sock is None:
            return
        try:
            self._call({"op": "close"})
        except (OSError, PodServerError, ConnectionError):
            pass
        self.sock.close()
        self.sock = None


__all__ = ["PodClient", "PodServerError", "PodServerGone", "ENV_POD_SERVER", "ENV_POD_CU_MASK", "ENV_POD_TOKEN"]
