/*
 * ClonosEngine -- Java facade over libclonos_engine.so (include/clonos_engine.h) through
 * jni/clonos_jni.c.  One engine per TaskManager per GPU; it owns the HBM segment pool
 * that replaces the NetworkBufferPool-backed determinant buffers
 * (JobCausalLogFactory.java:56-67).  Every native method returns a status (0 = OK);
 * check() turns a non-zero status into the exception the reference throws at the same
 * point (see INTEGRATION.md, "Errors").
 *
 * Source-only: this container has no JDK, so the binding is not compiled here.
 */
package org.apache.flink.runtime.causal.engine;

import org.apache.flink.runtime.causal.determinant.CorruptDeterminantArrayException;

import java.nio.ByteBuffer;
import java.util.NoSuchElementException;

public final class ClonosEngine implements AutoCloseable {

	static {
		System.loadLibrary("clonos_jni"); // links against libclonos_engine.so
	}

	public static final int CLG_OK = 0;
	public static final int CLG_E_INVALID_ARG = -1;
	public static final int CLG_E_CORRUPT_TAG = -2;
	public static final int CLG_E_TRUNCATED = -3;
	public static final int CLG_E_BAD_ENUM = -4;
	public static final int CLG_E_NEG_LEN = -5;
	public static final int CLG_E_BAD_SERIAL = -6;
	public static final int CLG_E_CONSUMER_BACKWARDS = -7;
	public static final int CLG_E_NO_CONSUMER = -8;
	public static final int CLG_E_GAP = -9;
	public static final int CLG_E_NOSPACE = -10;
	public static final int CLG_E_CAPACITY = -11;
	public static final int CLG_E_STATE = -12;
	public static final int CLG_E_DEVICE = -13;
	public static final int CLG_E_NO_LOG = -14;
	public static final int CLG_E_NOT_BUFFER_BUILT = -15;
	public static final int CLG_E_EPOCH_GAP = -16;
	// in-flight log types (InFlightLogConfig.java:44, taskmanager.inflight.type) and replay flags
	public static final int CLG_IFL_IN_MEMORY = 0;
	public static final int CLG_IFL_SPILLABLE = 1;
	public static final int CLG_IFL_CONTINUE = 1;
	public static final int CLG_IFL_NULL_ITERATOR = 1;
	public static final int CLG_IFL_REPLAYING = 2;

	/** The engine's default job (clg_config sharing depth). */
	public static final int DEFAULT_JOB = 0;

	private final long handle; // clg_engine*

	public ClonosEngine(int segmentBytes, int poolSegments, int device, int sharingDepth) {
		this(segmentBytes, poolSegments, device, sharingDepth, 0, 0);
	}

	/** inFlightSegmentBytes / inFlightPoolSegments: the in-flight log's own HBM pool (0: 32 KiB x 4096). */
	public ClonosEngine(int segmentBytes, int poolSegments, int device, int sharingDepth, int inFlightSegmentBytes,
						int inFlightPoolSegments) {
		long[] out = new long[1];
		check(nCreate(segmentBytes, poolSegments, device, sharingDepth, inFlightSegmentBytes, inFlightPoolSegments, out));
		this.handle = out[0];
	}

	public long handle() {
		return handle;
	}

	/** A JobCausalLog's scope on this engine (JobCausalLogFactory.java:56-67): JobID + its
	 *  ExecutionConfig.determinantSharingDepth.  Returns the job slot. */
	public int openJob(long jobIdLower, long jobIdUpper, int sharingDepth) {
		int[] out = new int[1];
		check(nJobOpen(handle, jobIdLower, jobIdUpper, sharingDepth, out));
		return out[0];
	}

	public void closeJob(int job) {
		check(nJobClose(handle, job));
	}

	/** CausalLogID fields (CausalLogID.java:38-60) of a log of `job` -> u32 log handle. */
	public int openLog(int job, short vertexId, boolean isMain, long irpLower, long irpUpper, byte subpartition) {
		int[] out = new int[1];
		check(nLogOpen(handle, job, vertexId, isMain, irpLower, irpUpper, subpartition, out));
		return out[0];
	}

	/** JobCausalLogImpl.notifyCheckpointComplete :230-246: the job's CAS + fan-out to its logs. */
	public boolean truncateAll(int job, long checkpointId) {
		int[] applied = new int[1];
		check(nTruncateAll(handle, job, checkpointId, applied));
		return applied[0] != 0;
	}

	/** The digests {hash, len} of getDeterminants(startEpochs[i]) of logs[i], computed on the device
	 *  (clg_digest_logs): 2 longs per log.  Two logs are equal only when both words are. */
	public long[] digestLogs(int[] logs, long[] startEpochs) {
		long[] out = new long[2 * logs.length];
		check(nDigestLogs(handle, logs, startEpochs, out));
		return out;
	}

	/** The same digests of spans of a direct buffer (clg_digest_spans). */
	public long[] digestSpans(ByteBuffer direct, long[] offs, long[] lens) {
		long[] out = new long[2 * offs.length];
		check(nDigestSpans(handle, direct, offs, lens, out));
		return out;
	}

	/** Where getDeterminants(startEpochs[i]) of logs[i] leaves span i = direct[offs[i], offs[i] + lens[i])
	 *  (clg_diff_logs): 3 longs per log, {lcp, lenLog, lenRef}.  lcp is the number of leading bytes the
	 *  two have in common; they are equal when all three words are. */
	public long[] diffLogs(int[] logs, long[] startEpochs, ByteBuffer direct, long[] offs, long[] lens) {
		long[] out = new long[3 * logs.length];
		check(nDiffLogs(handle, logs, startEpochs, direct, offs, lens, out));
		return out;
	}

	/** The digests of getDeterminants(startEpochs[i]) of logs[i] at each of its cut lengths
	 *  cuts[cutFirst[i] .. cutFirst[i + 1]) (not decreasing; unsigned), the range read once
	 *  (clg_digest_prefixes): 2 longs per cut, {hash, min(cut, length)}.  The holder of the longer copy of
	 *  a log checks with it that the shorter copy is a prefix: its row at the other side's length must
	 *  equal the other side's digest -- what the merge by length (DeterminantResponseEvent.java:137-146)
	 *  and processUpstreamDelta's offset dedup take for granted. */
	public long[] digestPrefixes(int[] logs, long[] startEpochs, long[] cutFirst, int[] cuts) {
		long[] out = new long[2 * cuts.length];
		check(nDigestPrefixes(handle, logs, startEpochs, cutFirst, cuts, out));
		return out;
	}

	/** One row per epoch of getDeterminants(startEpochs[i]) of logs[i], the digest of the range up to that
	 *  epoch's end (clg_digest_epochs).  Returns {first (n + 1 longs), epochIds, rows (2 longs each)}:
	 *  request i's rows are first[i] .. first[i + 1].  Two copies part in the first epoch whose rows differ. */
	public long[][] digestEpochs(int[] logs, long[] startEpochs) {
		long[] first = new long[logs.length + 1];
		long[] total = new long[1];
		check(nDigestEpochs(handle, logs, startEpochs, first, null, null, total));
		long[] ids = new long[(int) total[0]];
		long[] out = new long[2 * ids.length];
		if (ids.length > 0) {
			check(nDigestEpochs(handle, logs, startEpochs, first, ids, out, total));
		}
		return new long[][] {first, ids, out};
	}

	/** getDeterminants(startEpochs[i]) of logs[i] decoded on the device and delivered as typed columns
	 *  (clg_decode_logs_columns): the channels as bytes, the timestamps as longs, the random numbers and
	 *  buffer sizes as ints, each in record order, plus the tag stream that interleaves them -- what
	 *  LogReplayerImpl (LogReplayerImpl.java:61-119) consumes one value at a time.  Two native calls: sizes,
	 *  then the columns into direct buffers of exactly those sizes.  A decode error keeps each span's
	 *  records up to its first error; EngineDecodedColumns.errStatus() then says so. */
	public EngineDecodedColumns decodeLogsColumns(int[] logs, long[] startEpochs) {
		long[] res = new long[10];
		long[] spanBase = new long[5 * (logs.length + 1)];
		int st = nDecodeLogsColumns(handle, logs, startEpochs, null, null, null, null, null, null, null, null, null,
			null, null, null, res, spanBase);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st); // engine failure, not a decode error
		}
		EngineDecodedColumns c = new EngineDecodedColumns(res, logs.length);
		st = nDecodeLogsColumns(handle, logs, startEpochs, c.tag, c.order, c.timestamp, c.rng, c.bufferBuilt, c.wIdx,
			c.wRc, c.wV1, c.wVarOff, c.wVarLen, c.wSub, c.wV0, res, c.spanBase);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st);
		}
		c.setResult(res);
		return c;
	}

	/** decodeLogsColumns, and with withPayloads the payload column too (clg_decode_logs_columns_var): the
	 *  names, storage references and java streams of the wide rows packed in row order, gathered on the
	 *  device from the logs' segments -- EngineDecodedColumns.payload(k) is row k's bytes, and no log is
	 *  copied to the host for them.  Two native calls: sizes (of the columns and the payloads), then both. */
	public EngineDecodedColumns decodeLogsColumns(int[] logs, long[] startEpochs, boolean withPayloads) {
		if (!withPayloads) {
			return decodeLogsColumns(logs, startEpochs);
		}
		long[] res = new long[13];
		long[] spanBase = new long[5 * (logs.length + 1)];
		int st = nDecodeLogsColumnsVar(handle, logs, startEpochs, null, null, null, null, null, null, null, null, null,
			null, null, null, null, null, res, spanBase);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st); // engine failure, not a decode error
		}
		EngineDecodedColumns c = new EngineDecodedColumns(res, logs.length);
		c.allocatePayloads(res[10], res[11]);
		st = nDecodeLogsColumnsVar(handle, logs, startEpochs, c.tag, c.order, c.timestamp, c.rng, c.bufferBuilt, c.wIdx,
			c.wRc, c.wV1, c.wVarOff, c.wVarLen, c.wSub, c.wV0, c.var, c.varPos, res, c.spanBase);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st);
		}
		c.setResult(res);
		return c;
	}

	/** decodeLogsColumns with the five narrow columns delivered bit-packed (clg_decode_logs_columns_packed):
	 *  tags, channels, timestamps, random numbers and buffer sizes cross the link as the bits they hold, in
	 *  blocks of 1024 values, and EnginePackedColumns.cursor(s) pops them one typed value at a time, as
	 *  LogReplayerImpl does (LogReplayerImpl.java:61-119), without unpacking whole arrays.  The wide rows and
	 *  (withPayloads) the payload column come as decodeLogsColumns delivers them.  Two native calls: every
	 *  size, then the buffers. */
	public EnginePackedColumns decodeLogsColumnsPacked(int[] logs, long[] startEpochs, boolean withPayloads) {
		long[] res = new long[25];
		long[] spanBase = new long[5 * (logs.length + 1)];
		int st = nDecodeLogsColumnsPacked(handle, logs, startEpochs, null, null, null, null, null, null, null, null,
			null, null, null, withPayloads, res, spanBase);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st); // engine failure, not a decode error
		}
		EnginePackedColumns c = new EnginePackedColumns(res, logs.length, withPayloads);
		st = nDecodeLogsColumnsPacked(handle, logs, startEpochs, c.desc, c.bits, c.wIdx, c.wRc, c.wV1, c.wVarOff,
			c.wVarLen, c.wSub, c.wV0, c.var, c.varPos, withPayloads, res, c.spanBase);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st);
		}
		c.setResult(res);
		return c;
	}

	/**
	 * decodeLogsColumnsPacked with the wide rows delivered packed as well (clg_decode_logs_columns_packed_wide):
	 * no plain wide row and no payload position crosses the link.  EnginePackedWide.narrow holds the five
	 * narrow streams and the span bases, EnginePackedWide.cursor(s) pops span s's wide rows one at a time.
	 * Two native calls: the sizes, then the bytes.
	 */
	public EnginePackedWide decodeLogsColumnsPackedWide(int[] logs, long[] startEpochs, boolean withPayloads) {
		long[] res = new long[EnginePackedWide.R_LEN];
		long[] spanBase = new long[5 * (logs.length + 1)];
		int st = nDecodeLogsColumnsPackedWide(handle, logs, startEpochs, null, null, null, null, null, withPayloads,
			res, spanBase);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st); // engine failure, not a decode error
		}
		EnginePackedWide c = new EnginePackedWide(res, logs.length, withPayloads);
		st = nDecodeLogsColumnsPackedWide(handle, logs, startEpochs, c.narrow.desc, c.narrow.bits, c.desc, c.bits,
			c.var, withPayloads, res, c.narrow.spanBase);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st);
		}
		c.setResult(res);
		return c;
	}

	/**
	 * The log bytes of typed columns that carry their payload column (clg_encode_columns), encoded on the
	 * device from the columns as they are: the inverse of decodeLogsColumns(logs, startEpochs, true).  Span
	 * s's bytes are [spanByteBase[s], spanByteBase[s + 1]) of the returned buffer when spanByteBase
	 * (cols.spans() + 1 longs, may be null) is given.  Two native calls: the size, then the bytes.
	 */
	public ByteBuffer encodeColumns(EngineDecodedColumns cols, long[] spanByteBase) {
		if (!cols.hasPayloads()) {
			throw new IllegalStateException("decoded without payloads");
		}
		final long[] res = new long[3];
		final long[] sbb = spanByteBase != null ? spanByteBase : new long[cols.spans() + 1];
		check(nEncodeColumns(handle, cols.tag, cols.order, cols.timestamp, cols.rng, cols.bufferBuilt, cols.wIdx,
			cols.wRc, cols.wV1, cols.wVarLen, cols.wSub, cols.wV0, cols.var, cols.varPos, cols.spanBase,
			cols.records(), null, sbb, res));
		final ByteBuffer out = ByteBuffer.allocateDirect((int) Math.max(1, res[0]));
		check(nEncodeColumns(handle, cols.tag, cols.order, cols.timestamp, cols.rng, cols.bufferBuilt, cols.wIdx,
			cols.wRc, cols.wV1, cols.wVarLen, cols.wSub, cols.wV0, cols.var, cols.varPos, cols.spanBase,
			cols.records(), out, sbb, res));
		out.limit((int) res[0]);
		return out;
	}

	public ByteBuffer encodeColumns(EngineDecodedColumns cols) {
		return encodeColumns(cols, null);
	}

	/**
	 * The batched write path from columns (clg_append_columns): the columns are encoded on the device and
	 * span s becomes one appendDeterminant batch of logs[s] in epochs[s], scattered into the log's segments
	 * without an encoded byte crossing the link.  Returns per span the bytes appended, or the span's
	 * (negative) status when it was not applied (CLG_E_NO_LOG, CLG_E_NOSPACE: the caller applies
	 * backpressure and sends that span again); the other spans are applied.  Invalid columns throw before
	 * any log changes.
	 */
	public long[] appendColumns(int[] logs, long[] epochs, EngineDecodedColumns cols) {
		if (!cols.hasPayloads()) {
			throw new IllegalStateException("decoded without payloads");
		}
		final long[] spanBytes = new long[logs.length];
		final int[] status = new int[logs.length];
		check(nAppendColumns(handle, logs, epochs, cols.tag, cols.order, cols.timestamp, cols.rng, cols.bufferBuilt,
			cols.wIdx, cols.wRc, cols.wV1, cols.wVarLen, cols.wSub, cols.wV0, cols.var, cols.varPos, cols.spanBase,
			cols.records(), spanBytes, status));
		for (int s = 0; s < logs.length; s++) {
			if (status[s] != CLG_OK) {
				spanBytes[s] = status[s];
			}
		}
		return spanBytes;
	}

	/**
	 * appendColumns for packed columns (clg_append_columns_packed): desc and bits go up as they were
	 * delivered -- the narrow form is what crosses the link -- and are checked and unpacked on the device
	 * before the existing encode and scatter run.  The packed bytes are not trusted: a malformed layout,
	 * block or value throws before any log changes, its message carrying {bad_what, bad_stream,
	 * bad_block}, which are also left in lastUnpackBad().  Returns per span the bytes appended or the
	 * span's (negative) status, as appendColumns does.
	 */
	public long[] appendColumnsPacked(int[] logs, long[] epochs, EnginePackedColumns cols) {
		if (!cols.hasPayloads()) {
			throw new IllegalStateException("decoded without payloads");
		}
		final long[] spanBytes = new long[logs.length];
		final int[] status = new int[logs.length];
		final long[] bad = new long[3];
		final int st = nAppendColumnsPacked(handle, logs, epochs, cols.desc, cols.bits, cols.nVal, cols.blkBase, cols.nBits,
			cols.wIdx, cols.wRc, cols.wV1, cols.wVarLen, cols.wSub, cols.wV0, cols.var, cols.varPos, cols.spanBase,
			spanBytes, status, bad);
		lastUnpackBad = bad;
		if (st != CLG_OK && bad[0] != 0) {
			throw new IllegalArgumentException("packed columns: bad_what " + bad[0] + ", bad_stream " + bad[1]
				+ ", bad_block " + bad[2] + ": " + nLastError());
		}
		check(st);
		for (int s = 0; s < logs.length; s++) {
			if (status[s] != CLG_OK) {
				spanBytes[s] = status[s];
			}
		}
		return spanBytes;
	}

	/**
	 * appendColumnsPacked with the wide rows packed as well (clg_append_columns_packed_wide): what
	 * decodeLogsColumnsPackedWide delivered goes up as it is -- both packed forms and the payload bytes --
	 * and is checked and unpacked on the device, where pos is rebuilt; no plain column, wide row or pos
	 * exists on this side.  cols is wide.narrow.  A finding throws as appendColumnsPacked's does; one in
	 * the wide rows reports bad_stream 32 + its stream, and a row whose w_idx names no wide record of
	 * its kind is {VALUE, 33, row / 1024}.
	 */
	public long[] appendColumnsPackedWide(int[] logs, long[] epochs, EnginePackedColumns cols, EnginePackedWide wide) {
		if (!wide.hasPayloads()) {
			throw new IllegalStateException("decoded without payloads");
		}
		if (cols != wide.narrow) {
			throw new IllegalArgumentException("cols must be wide.narrow");
		}
		final long[] spanBytes = new long[logs.length];
		final int[] status = new int[logs.length];
		final long[] bad = new long[3];
		final int st = nAppendColumnsPackedWide(handle, logs, epochs, cols.desc, cols.bits, cols.nVal, cols.blkBase, cols.nBits,
			wide.desc, wide.bits, wide.nVal, wide.blkBase, wide.nBits, wide.var, wide.nVar, cols.spanBase, spanBytes, status, bad);
		lastUnpackBad = bad;
		if (st != CLG_OK && bad[0] != 0) {
			throw new IllegalArgumentException("packed columns: bad_what " + bad[0] + ", bad_stream " + bad[1]
				+ ", bad_block " + bad[2] + ": " + nLastError());
		}
		check(st);
		for (int s = 0; s < logs.length; s++) {
			if (status[s] != CLG_OK) {
				spanBytes[s] = status[s];
			}
		}
		return spanBytes;
	}

	private long[] lastUnpackBad = new long[3];

	/** {bad_what, bad_stream, bad_block} of the last appendColumnsPacked / appendColumnsPackedWide call (all 0, 0, ~0 or zero when clean). */
	public long[] lastUnpackBad() {
		return lastUnpackBad.clone();
	}

	/**
	 * Replay preparation for one failed task with the main log delivered as typed columns and the payload
	 * column (clg_replay_prepare_columns), in ONE native call: the buffers are sized by bounds no main log
	 * of mainLen bytes can exceed (the shortest record of each class: ORDER 2 B, TIMESTAMP 9, RNG and
	 * BUFFER_BUILT 5, wide 6), so no sizes-only call comes first.  buffers / lens / subpartitions /
	 * bufferSizes / subpartitionResults are nReplayPrepare's.  A decode error of the main log is in the
	 * result's errStatus(); the columns then hold the records before it.
	 */
	public EngineDecodedColumns replayPrepareColumns(short vertexId, ByteBuffer[] buffers, int[] lens,
													 long[] subpartitions, ByteBuffer bufferSizes,
													 long[] subpartitionResults) {
		final long mainLen = lens[0];
		final long[] res = new long[13];
		final long[] bounds = {mainLen / 2 + 1, mainLen / 2 + 1, mainLen / 9 + 1, mainLen / 5 + 1, mainLen / 5 + 1,
			mainLen / 6 + 1, CLG_OK, 0, 0, 0};
		final EngineDecodedColumns c = new EngineDecodedColumns(bounds, 1);
		c.allocatePayloads(mainLen / 6 + 1, mainLen + 1);
		final int st = nReplayPrepareColumns(handle, vertexId, buffers, lens, subpartitions, c.tag, c.order, c.timestamp,
			c.rng, c.bufferBuilt, c.wIdx, c.wRc, c.wV1, c.wVarOff, c.wVarLen, c.wSub, c.wV0, c.var, c.varPos, res,
			c.spanBase, bufferSizes, subpartitionResults);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st); // an engine failure, not a decode error of the main log
		}
		c.setResult(res);
		return c;
	}

	/**
	 * Replay preparation for one failed task with the main log delivered as packed typed columns
	 * (clg_replay_prepare_columns_packed): the five narrow columns and the wide rows both bit-packed, the
	 * payload bytes without pos -- what the cursors of EnginePackedColumns and EnginePackedWide pop from.
	 * Two native calls, as decodeLogsColumnsPackedWide makes: the sizes, then the blocks into buffers of
	 * exactly those sizes.  buffers / lens / subpartitions / bufferSizes / subpartitionResults are
	 * nReplayPrepare's.  A decode error of the main log is in the result's narrow.errStatus(); the blocks
	 * then hold the records before it.  result.narrow is the EnginePackedColumns.
	 */
	public EnginePackedWide replayPrepareColumnsPacked(short vertexId, ByteBuffer[] buffers, int[] lens,
													   long[] subpartitions, ByteBuffer bufferSizes,
													   long[] subpartitionResults, boolean withPayloads) {
		final long[] res = new long[EnginePackedWide.R_LEN];
		final long[] spanBase = new long[5 * 2];
		int st = nReplayPrepareColumnsPacked(handle, vertexId, buffers, lens, subpartitions, null, null, null, null,
			null, withPayloads, res, spanBase, bufferSizes, subpartitionResults);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st); // an engine failure, not a decode error of the main log
		}
		final EnginePackedWide c = new EnginePackedWide(res, 1, withPayloads);
		st = nReplayPrepareColumnsPacked(handle, vertexId, buffers, lens, subpartitions, c.narrow.desc, c.narrow.bits,
			c.desc, c.bits, c.var, withPayloads, res, c.narrow.spanBase, bufferSizes, subpartitionResults);
		if (st != CLG_OK && res[6] == CLG_OK) {
			check(st);
		}
		c.setResult(res);
		return c;
	}

	@Override
	public void close() {
		nDestroy(handle);
	}

	public static void check(int status) {
		if (status == CLG_OK) {
			return;
		}
		throw toException(status, nLastError());
	}

	/** The exception the reference throws at the point the status stands for. */
	public static RuntimeException toException(int status, String msg) {
		switch (status) {
			case CLG_E_CORRUPT_TAG: // SimpleDeterminantEncoder.decodeNext :92
				return new CorruptDeterminantArrayException(tagOf(msg));
			case CLG_E_BAD_ENUM: // ProcessingTimeCallbackID.Type.values()[ord] / CheckpointType.values()[ord]
				return new ArrayIndexOutOfBoundsException(msg);
			case CLG_E_NEG_LEN: // new byte[negative] (:235, :282)
				return new NegativeArraySizeException(msg);
			case CLG_E_TRUNCATED: // ByteBuf.readX past writerIndex
			case CLG_E_GAP: // ThreadCausalLogImpl.processUpstreamDelta: delta.readerIndex(< 0) (:143)
			case CLG_E_STATE: // makeDeltaUnsafe / getDeterminants index checks
				return new IndexOutOfBoundsException(msg);
			case CLG_E_CONSUMER_BACKWARDS: // ThreadCausalLogImpl.java:215-218
				return new RuntimeException("Consumer went backwards: " + msg);
			case CLG_E_NO_CONSUMER: // :245 / :256 dereference a missing ConsumerOffset
			case CLG_E_EPOCH_GAP: // ReplayIterator :133 / SpilledReplayIterator.EpochCursor (log.get(epoch) == null)
			case CLG_E_NO_LOG: // flatThreadCausalLogs.get(id) == null
				return new NullPointerException(msg);
			case CLG_E_NOT_BUFFER_BUILT: // ReplayingState.SubpartitionRecoveryThread :172-177
				return new RuntimeException("Subpartition has corrupt recovery buffer, expected buffer built: " + msg);
			case CLG_E_INVALID_ARG:
				return new IllegalArgumentException(msg);
			default: // CLG_E_NOSPACE (callers retry), CLG_E_CAPACITY (callers resize), CLG_E_DEVICE
				return new IllegalStateException("clonos engine status " + status + ": " + msg);
		}
	}

	/** The tag byte clg_last_error reports for CLG_E_CORRUPT_TAG ("... (tag N)"). */
	private static byte tagOf(String msg) {
		int i = msg.lastIndexOf("tag ");
		if (i < 0) {
			return 0;
		}
		int j = i + 4;
		while (j < msg.length() && (Character.isDigit(msg.charAt(j)) || msg.charAt(j) == '-')) {
			j++;
		}
		try {
			return (byte) Integer.parseInt(msg.substring(i + 4, j));
		} catch (NumberFormatException e) {
			return 0;
		}
	}

	/** In-flight iterator statuses (InMemorySubpartitionInFlightLogger.ReplayIterator): a skip past
	 *  the end is ListIterator.next()'s NoSuchElementException; a start epoch that is absent
	 *  (currentIterator == null) or a gap (logToReplay.get(++currentKey) == null) is a
	 *  NullPointerException.  clg_last_error names the case. */
	public static RuntimeException inFlightException(int status, String msg) {
		if (status == CLG_E_STATE && msg.contains("past the end")) {
			return new NoSuchElementException(msg);
		}
		if (status == CLG_E_STATE || status == CLG_E_EPOCH_GAP) {
			return new NullPointerException(msg);
		}
		return toException(status, msg);
	}

	// ---- natives (jni/clonos_jni.c) ------------------------------------------------------
	static native int nCreate(int segmentBytes, int poolSegments, int device, int sharingDepth, int iflSegmentBytes,
							  int iflPoolSegments, long[] out);
	static native void nDestroy(long engine);
	static native String nLastError();
	static native int nJobOpen(long engine, long jobIdLower, long jobIdUpper, int sharingDepth, int[] out);
	static native int nJobClose(long engine, int job);
	static native int nLogOpen(long engine, int job, short vertexId, boolean isMain, long irpLower, long irpUpper,
							   byte subpartition, int[] out);
	static native int nLogClose(long engine, int log);
	// in-flight (data) log, InMemorySubpartitionInFlightLogger (inflightlogging/, :28-207) or
	// SpillableSubpartitionInFlightLogger (:45-341): type CLG_IFL_IN_MEMORY / CLG_IFL_SPILLABLE
	static native int nIflOpen(long engine, int type, int[] out);
	static native int nIflClose(long engine, int ifl);
	static native int nIflLog(long engine, int ifl, long epoch, ByteBuffer direct, int off, int len);
	/** n buffers staged back to back in `direct` (lens[i] bytes, epoch epochs[i]), logged in order. */
	static native int nIflLogBatch(long engine, int ifl, long[] epochs, int[] lens, ByteBuffer direct, int n);
	static native int nIflNotifyCheckpointComplete(long engine, int ifl, long checkpointId);
	/** res = {status, n_buffers, remaining, len, total, total_buffers, end_epoch, flags}; sizes (i32)
	 *  and epochs (i64, native order) receive one entry per buffer.  maxBuffers (0: all) and
	 *  flags CLG_IFL_CONTINUE (take from the current iterator) apply to spillable logs only. */
	static native int nIflReplay(long engine, int ifl, long startEpoch, int ignoreBuffers, int maxBuffers, int flags,
		ByteBuffer out, ByteBuffer sizes, ByteBuffer epochs, long[] res);
	/** bytes = direct buffer holding encoded records (SimpleDeterminantEncoder.encodeTo). */
	static native int nAppend(long engine, int log, long epoch, ByteBuffer direct, int off, int len);
	static native int nUpstreamDelta(long engine, int log, long epoch, int offsetFromEpoch, ByteBuffer direct,
									 int off, int len);
	static native int nLogLength(long engine, int log, int[] out);
	static native int nHasDelta(long engine, int log, long chLo, long chHi, long epoch, int[] out);
	static native int nOffsetFromEpoch(long engine, int log, long chLo, long chHi, int[] out);
	/** out[0] = bytes written, or the required size with CLG_E_CAPACITY. */
	static native int nGetDelta(long engine, int log, long chLo, long chHi, long epoch, ByteBuffer direct,
								int[] out);
	static native int nGetDeterminants(long engine, int log, long startEpoch, ByteBuffer direct, int[] out);
	static native int nNotifyCheckpointComplete(long engine, int log, long checkpointId);
	static native int nUnregisterConsumer(long engine, int log, long chLo, long chHi);
	static native int nTruncateAll(long engine, int job, long checkpointId, int[] applied);

	// batched paths: LogReplayerImpl / ReplayingState decode, the piggyback serde, replay-prep
	static native int nDecodeLogs(long engine, int[] logs, long[] startEpochs, ByteBuffer off, ByteBuffer tag,
								  ByteBuffer v0, ByteBuffer wIdx, ByteBuffer wRc, ByteBuffer wV1, ByteBuffer wVarOff,
								  ByteBuffer wVarLen, ByteBuffer wSub, long[] result, long[] spanRecBase);
	/** clg_decode_logs_columns: typed columns into direct buffers (all null: sizes only); result = {nRec, nOrder,
	 *  nTimestamp, nRng, nBufferBuilt, nWide, errStatus, errSpan, errOff, errTag}; spanBase = 5 (n + 1) longs. */
	static native int nDecodeLogsColumns(long engine, int[] logs, long[] startEpochs, ByteBuffer tag, ByteBuffer order,
										 ByteBuffer timestamp, ByteBuffer rng, ByteBuffer bufferBuilt, ByteBuffer wIdx,
										 ByteBuffer wRc, ByteBuffer wV1, ByteBuffer wVarOff, ByteBuffer wVarLen,
										 ByteBuffer wSub, ByteBuffer wV0, long[] result, long[] spanBase);
	/** clg_decode_logs_columns_var: nDecodeLogsColumns plus the payload column (var, and pos = nWide + 1 longs);
	 *  result = nDecodeLogsColumns' ten entries, then {nRows, nVar, badRow}. */
	static native int nDecodeLogsColumnsVar(long engine, int[] logs, long[] startEpochs, ByteBuffer tag, ByteBuffer order,
											ByteBuffer timestamp, ByteBuffer rng, ByteBuffer bufferBuilt, ByteBuffer wIdx,
											ByteBuffer wRc, ByteBuffer wV1, ByteBuffer wVarOff, ByteBuffer wVarLen,
											ByteBuffer wSub, ByteBuffer wV0, ByteBuffer var, ByteBuffer varPos,
											long[] result, long[] spanBase);
	/** clg_decode_logs_columns_packed: desc (32-byte block descriptors) and bits, the wide rows, the payload
	 *  column when withPayloads (all buffers null: sizes only); result = nDecodeLogsColumnsVar's thirteen
	 *  entries, then {nVal[5], blkBase[6], nBits}. */
	static native int nDecodeLogsColumnsPacked(long engine, int[] logs, long[] startEpochs, ByteBuffer desc,
											   ByteBuffer bits, ByteBuffer wIdx, ByteBuffer wRc, ByteBuffer wV1,
											   ByteBuffer wVarOff, ByteBuffer wVarLen, ByteBuffer wSub, ByteBuffer wV0,
											   ByteBuffer var, ByteBuffer varPos, boolean withPayloads, long[] result,
											   long[] spanBase);
	/** clg_decode_logs_columns_packed_wide: result[0..24] as nDecodeLogsColumnsPacked, then the wide pack's
	 *  n_val[26], blk_base[27], n_bits and bad_row (80 longs); every buffer null: sizes only. */
	static native int nDecodeLogsColumnsPackedWide(long engine, int[] logs, long[] startEpochs, ByteBuffer desc,
												   ByteBuffer bits, ByteBuffer wideDesc, ByteBuffer wideBits,
												   ByteBuffer var, boolean withPayloads, long[] result,
												   long[] spanBase);
	/** clg_encode_columns over host columns; out null: sizes only.  result = {n_bytes, bad_what, bad_index}. */
	static native int nEncodeColumns(long engine, ByteBuffer tag, ByteBuffer order, ByteBuffer timestamp, ByteBuffer rng,
									 ByteBuffer bufferBuilt, ByteBuffer wIdx, ByteBuffer wRc, ByteBuffer wV1,
									 ByteBuffer wVarLen, ByteBuffer wSub, ByteBuffer wV0, ByteBuffer var, ByteBuffer varPos,
									 long[] spanBase, long nRec, ByteBuffer out, long[] spanByteBase, long[] result);
	/** clg_append_columns: spanBytes and status hold an entry per span. */
	static native int nAppendColumnsPacked(long engine, int[] logs, long[] epochs, ByteBuffer desc, ByteBuffer bits,
		long[] nVal, long[] blkBase, long nBits, ByteBuffer wIdx, ByteBuffer wRc, ByteBuffer wV1, ByteBuffer wVarLen,
		ByteBuffer wSub, ByteBuffer wV0, ByteBuffer var, ByteBuffer varPos, long[] spanBase, long[] spanBytes,
		int[] status, long[] bad);
	/** clg_append_columns_packed_wide: both packed forms and the payload bytes; no rows and no pos. */
	static native int nAppendColumnsPackedWide(long engine, int[] logs, long[] epochs, ByteBuffer desc, ByteBuffer bits,
		long[] nVal, long[] blkBase, long nBits, ByteBuffer wDesc, ByteBuffer wBits, long[] wNVal, long[] wBlkBase,
		long wNBits, ByteBuffer var, long nVar, long[] spanBase, long[] spanBytes, int[] status, long[] bad);

	static native int nAppendColumns(long engine, int[] logs, long[] epochs, ByteBuffer tag, ByteBuffer order,
									 ByteBuffer timestamp, ByteBuffer rng, ByteBuffer bufferBuilt, ByteBuffer wIdx,
									 ByteBuffer wRc, ByteBuffer wV1, ByteBuffer wVarLen, ByteBuffer wSub, ByteBuffer wV0,
									 ByteBuffer var, ByteBuffer varPos, long[] spanBase, long nRec, long[] spanBytes,
									 int[] status);
	/** clg_decode_logs_async: ctx[0] = a handle for nDecodeWait (the buffers stay reachable until then). */
	static native int nDecodeLogsAsync(long engine, int[] logs, long[] startEpochs, ByteBuffer off, ByteBuffer tag,
									   ByteBuffer v0, ByteBuffer wIdx, ByteBuffer wRc, ByteBuffer wV1, ByteBuffer wVarOff,
									   ByteBuffer wVarLen, ByteBuffer wSub, long[] ctx);
	/** clg_decode_wait: completes the decode nDecodeLogsAsync queued; result as nDecodeLogs. */
	static native int nDecodeWait(long engine, long ctx, long[] result, long[] spanRecBase);
	/** One span of host bytes decoded on the GPU (clg_decode_host); result as nDecodeLogs. */
	static native int nDecodeHost(long engine, ByteBuffer bytes, int off, int len, ByteBuffer recOff, ByteBuffer tag,
								  ByteBuffer v0, ByteBuffer wIdx, ByteBuffer wRc, ByteBuffer wV1, ByteBuffer wVarOff,
								  ByteBuffer wVarLen, ByteBuffer wSub, long[] result);
	/** clg_digest_logs: out = {hash, len} of getDeterminants(startEpochs[i]) of logs[i] (2 n longs). */
	static native int nDigestLogs(long engine, int[] logs, long[] startEpochs, long[] out);
	/** clg_digest_spans: span i = direct[offs[i], offs[i] + lens[i]); out as nDigestLogs. */
	static native int nDigestSpans(long engine, ByteBuffer direct, long[] offs, long[] lens, long[] out);
	/** clg_diff_logs: out = {lcp, lenLog, lenRef} of logs[i] from startEpochs[i] against
	 *  direct[offs[i], offs[i] + lens[i]) (3 n longs). */
	static native int nDiffLogs(long engine, int[] logs, long[] startEpochs, ByteBuffer direct, long[] offs, long[] lens,
								long[] out);
	/** clg_digest_prefixes: out = {hash, len} per cut (2 longs each), cuts[cutFirst[i] .. cutFirst[i + 1]) request i's. */
	static native int nDigestPrefixes(long engine, int[] logs, long[] startEpochs, long[] cutFirst, int[] cuts,
									  long[] out);
	/** clg_digest_epochs: first = n + 1 longs, total = 1 long; epochIds and out null: sizes only, otherwise room
	 *  for epochIds.length rows (out: 2 longs per row). */
	static native int nDigestEpochs(long engine, int[] logs, long[] startEpochs, long[] first, long[] epochIds,
									long[] out, long[] total);
	/** out = {vertexId, isMain, irpLower, irpUpper, subpartition, job}. */
	static native int nLogGetId(long engine, int log, long[] out);
	static native int nEnrichBatch(long engine, int strategy, long[] requests, int[] logs, byte[] flags,
								   ByteBuffer out, long[] results, long[] total);
	static native int nProcessDelta(long engine, int job, int strategy, ByteBuffer msg, int off, int len,
									int[] handles, long[] result);
	static native int nReplayPrepare(long engine, short vertexId, ByteBuffer[] buffers, int[] lens, long[] subpartitions,
									 ByteBuffer off, ByteBuffer tag, ByteBuffer v0, ByteBuffer wIdx, ByteBuffer wRc,
									 ByteBuffer wV1, ByteBuffer wVarOff, ByteBuffer wVarLen, ByteBuffer wSub,
									 long[] result, ByteBuffer bufferSizes, long[] subpartitionResults);
	/** clg_replay_prepare_columns: nReplayPrepare's inputs, nDecodeLogsColumnsVar's outputs (result: 13 longs;
	 *  spanBase: 10), then nReplayPrepare's subpartition outputs. */
	static native int nReplayPrepareColumns(long engine, short vertexId, ByteBuffer[] buffers, int[] lens,
											long[] subpartitions, ByteBuffer tag, ByteBuffer order, ByteBuffer timestamp,
											ByteBuffer rng, ByteBuffer bufferBuilt, ByteBuffer wIdx, ByteBuffer wRc,
											ByteBuffer wV1, ByteBuffer wVarOff, ByteBuffer wVarLen, ByteBuffer wSub,
											ByteBuffer wV0, ByteBuffer var, ByteBuffer varPos, long[] result,
											long[] spanBase, ByteBuffer bufferSizes, long[] subpartitionResults);
	/** clg_replay_prepare_columns_packed: nReplayPrepare's inputs, nDecodeLogsColumnsPackedWide's outputs (result:
	 *  80 longs; spanBase: 10; every buffer null: the sizes only), then
	 *  nReplayPrepare's subpartition outputs. */
	static native int nReplayPrepareColumnsPacked(long engine, short vertexId, ByteBuffer[] buffers, int[] lens,
												  long[] subpartitions, ByteBuffer desc, ByteBuffer bits, ByteBuffer wdesc,
												  ByteBuffer wbits, ByteBuffer var, boolean withPayloads, long[] result,
												  long[] spanBase, ByteBuffer bufferSizes, long[] subpartitionResults);
}
