/*
 * EnginePackedWide -- a decoded batch of logs whose wide rows are packed as well (clg_packed_wide,
 * include/clonos_engine.h; the format: clonos_amd/csrc/pack_wide.h).  The narrow columns are an
 * EnginePackedColumns without wide rows (narrow); the wide rows are partitioned by record kind
 * (kind = tag - 3: SERIALIZABLE, TIMER_TRIGGER, SOURCE_CHECKPOINT, IGNORE_CHECKPOINT) and every
 * field of every kind is a stream of its own, packed block by block as the narrow streams are.
 *
 *   stream 0 KIND, 1 IDX, then 2 + 6 * kind + field with the fields RC, V1, VAR_OFF, VAR_LEN,
 *   SUB, V0; IDX, V1 and VAR_OFF are DELTA streams, V0 is DELTA for kinds 1 - 3 and FOR for
 *   kind 0, the rest are FOR
 *
 * LogReplayerImpl pops one determinant at a time (LogReplayerImpl.java:61-119), so nothing is
 * unpacked into arrays here: a Cursor pops the next wide row, its kind from KIND and its six
 * fields from its kind's streams at the kind's next rank, and keeps the running sum of the
 * lengths, which is the row's place in the payload column (pos is not delivered).  Where a span's
 * rows begin in each kind's streams and in the payload column is found once for all spans, in one
 * pass over KIND and the lengths, when the first cursor is asked for.
 *
 * Source-only: this container has no JDK, so the binding is not compiled here.
 */
package org.apache.flink.runtime.causal.engine;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

public final class EnginePackedWide {

	public static final int KINDS = 4, FIELDS = 6, STREAMS = 26, KIND = 0, IDX = 1;
	public static final int RC = 0, V1 = 1, VAR_OFF = 2, VAR_LEN = 3, SUB = 4, V0 = 5;
	static final int BLOCK = EnginePackedColumns.BLOCK, DESC_BYTES = EnginePackedColumns.DESC_BYTES;
	/** Offsets in nDecodeLogsColumnsPackedWide's result: n_val[26], blk_base[27], n_bits, bad_row. */
	static final int R_NVAL = 25, R_BLKBASE = 51, R_NBITS = 78, R_LEN = 80;

	/** The narrow columns, span bases and error fields; it holds no wide rows. */
	public final EnginePackedColumns narrow;
	final ByteBuffer desc, bits;
	ByteBuffer var;
	final long[] nVal = new long[STREAMS];
	final long[] blkBase = new long[STREAMS + 1];
	long nBits;
	/** The payload bytes in var (0 without payloads). */
	long nVar;

	/** Direct buffers of exactly the sizes a sizes-only call reported. */
	EnginePackedWide(long[] sizes, int nSpans, boolean withPayloads) {
		final long[] noWide = java.util.Arrays.copyOf(sizes, 25);
		noWide[5] = 0; // no plain wide rows are delivered
		this.narrow = new EnginePackedColumns(noWide, nSpans, false);
		this.desc = direct(DESC_BYTES * sizes[R_BLKBASE + STREAMS]);
		this.bits = direct(sizes[R_NBITS]);
		if (withPayloads) {
			this.var = direct(sizes[11]);
		}
		setResult(sizes);
	}

	private static ByteBuffer direct(long bytes) {
		return ByteBuffer.allocateDirect((int) Math.max(1, bytes)).order(ByteOrder.nativeOrder());
	}

	void setResult(long[] res) {
		narrow.setResult(res);
		System.arraycopy(res, R_NVAL, nVal, 0, STREAMS);
		System.arraycopy(res, R_BLKBASE, blkBase, 0, STREAMS + 1);
		this.nBits = res[R_NBITS];
		this.nVar = var != null ? res[11] : 0;
	}

	public static int stream(int kind, int field) {
		return 2 + FIELDS * kind + field;
	}

	/** The format's scheme table. */
	public static boolean isDelta(int stream) {
		if (stream < 2) {
			return stream == IDX;
		}
		final int kind = (stream - 2) / FIELDS, field = (stream - 2) % FIELDS;
		return field == V1 || field == VAR_OFF || (field == V0 && kind != 0);
	}

	public long wideRows() {
		return nVal[KIND];
	}

	public long rows(int kind) {
		return nVal[stream(kind, RC)];
	}

	public boolean hasPayloads() {
		return var != null;
	}

	/** The delivered size in bytes: the narrow descriptors and payload bits, the span bases, the wide
	 *  descriptors and payload bits, the payload bytes (narrow holds no wide rows: none are counted). */
	public long deliveredBytes() {
		final long n = DESC_BYTES * (narrow.blkBase[EnginePackedColumns.STREAMS] + blkBase[STREAMS]) + narrow.nBits + nBits
			+ 8L * narrow.spanBase.length;
		return var != null ? n + var.capacity() : n;
	}

	/** A wide row as the cursor pops it.  varPos is the row's first byte in the payload column. */
	public static final class Row {
		public int kind, rc, sub;
		public long idx, v1, varOff, varLen, v0, varPos;
	}

	/** The payload bytes of a popped row: a slice of the payload column, not a copy. */
	public ByteBuffer payload(Row r) {
		if (var == null) {
			throw new IllegalStateException("decoded without payloads");
		}
		final ByteBuffer d = var.duplicate();
		d.position((int) r.varPos);
		d.limit((int) (r.varPos + r.varLen));
		return d.slice();
	}

	/** Per span s (and s == spans(): the totals): the rows of each kind before it, KINDS longs a span,
	 *  and the payload bytes before it.  Built by index(). */
	private long[] spanRank, spanVarPos;

	/** One pass over all rows, KIND and VAR_LEN only: every span's place in the kinds' streams. */
	private void index() {
		final int n = narrow.spans();
		final long[] rank = new long[KINDS * (n + 1)], pos = new long[n + 1];
		final Stream kinds = new Stream(KIND);
		final Stream[] len = new Stream[KINDS];
		for (int t = 0; t < KINDS; t++) {
			len[t] = new Stream(stream(t, VAR_LEN));
		}
		final long[] r = new long[KINDS];
		long at = 0, row = 0;
		for (int s = 0; s <= n; s++) {
			for (final long end = narrow.base(s, EnginePackedColumns.WIDE); row < end; row++) {
				final int kind = (int) kinds.next();
				at += len[kind].next();
				r[kind]++;
			}
			System.arraycopy(r, 0, rank, KINDS * s, KINDS);
			pos[s] = at;
		}
		spanRank = rank;
		spanVarPos = pos;
	}

	/** A cursor over span s's wide rows, in row order. */
	public Cursor cursor(int s) {
		if (spanRank == null) {
			index();
		}
		return new Cursor(s);
	}

	/** One stream's position: the current block's descriptor, and for a DELTA stream the running value. */
	private final class Stream {
		final int stream;
		final boolean delta;
		long next;             // the next value's index in the stream
		long ref, pos, acc;    // the current block's reference and payload offset; the last DELTA value
		int width;
		long blockFirst = -1;  // the stream index of the current block's first value (-1: none loaded)
		long last = -2;        // the index of the value acc holds

		Stream(int stream) {
			this.stream = stream;
			this.delta = isDelta(stream);
		}

		private long field(long j) {
			if (width == 0) {
				return 0;
			}
			final long bit = j * width;
			final int at = (int) (pos + (bit >>> 6) * 8), sh = (int) (bit & 63);
			long v = bits.getLong(at) >>> sh;
			if (sh + width > 64) {
				v |= bits.getLong(at + 8) << (64 - sh);
			}
			return width == 64 ? v : v & ((1L << width) - 1);
		}

		private void load(long block) {
			final int d = (int) ((blkBase[stream] + block) * DESC_BYTES);
			ref = desc.getLong(d);
			acc = desc.getLong(d + 8);
			pos = desc.getLong(d + 16);
			width = desc.getInt(d + 24);
			blockFirst = block * BLOCK;
			last = blockFirst;
		}

		long next() {
			if (next >= nVal[stream]) {
				throw new IllegalStateException("stream " + stream + " is finished");
			}
			final long i = next++;
			final long block = i / BLOCK, k = i % BLOCK;
			if (!delta) {
				if (blockFirst != block * BLOCK) {
					load(block);
				}
				return ref + field(k);
			}
			if (blockFirst != block * BLOCK || last > i) {
				load(block);
			}
			for (long j = last - blockFirst + 1; j <= k; j++) { // (one step when the values are read in turn)
				acc += ref + field(j - 1);
			}
			last = i;
			return acc;
		}
	}

	public final class Cursor {
		private final Stream[] st = new Stream[STREAMS];
		private long row;
		private final long end;
		private long varPos;

		/** Span s's rows: every stream starts where index() found the span to begin (a DELTA stream
		 *  that starts inside a block runs up to its first value when it is first read). */
		Cursor(int s) {
			row = narrow.base(s, EnginePackedColumns.WIDE);
			end = narrow.base(s + 1, EnginePackedColumns.WIDE);
			varPos = spanVarPos[s];
			for (int c = 0; c < STREAMS; c++) {
				st[c] = new Stream(c);
				st[c].next = c < 2 ? row : spanRank[KINDS * s + (c - 2) / FIELDS];
			}
		}

		public boolean isFinished() {
			return row >= end;
		}

		/** The next wide row: its kind and its six fields (rc, v1, varOff, varLen, sub, v0), and w_idx. */
		public Row next(Row r) {
			if (row >= end) {
				throw new IllegalStateException("the span's wide rows are finished");
			}
			row++;
			r.kind = (int) st[KIND].next();
			r.idx = st[IDX].next();
			r.rc = (int) st[stream(r.kind, RC)].next();
			r.v1 = st[stream(r.kind, V1)].next();
			r.varOff = st[stream(r.kind, VAR_OFF)].next();
			r.varLen = st[stream(r.kind, VAR_LEN)].next();
			r.sub = (int) st[stream(r.kind, SUB)].next();
			r.v0 = st[stream(r.kind, V0)].next();
			r.varPos = varPos;
			varPos += r.varLen;
			return r;
		}

		public Row next() {
			return next(new Row());
		}
	}
}
