/*
 * strom_timelib.h -- date / time / timestamp functions (device)
 *
 * Role in the reference: opencl_timelib.h (types 102-120, casts 227-320,
 * date +/- int 326-410, date<->timestamp comparisons 413-660).  date is
 * days since 2000-01-01 (int32), time and timestamp are microseconds
 * (int64, HAVE_INT64_TIMESTAMP).  Anything that would overflow goes back
 * to the CPU (CpuReCheck) exactly as the arithmetic library does.
 */
#ifndef STROM_TIMELIB_DEVICE_H
#define STROM_TIMELIB_DEVICE_H

#define STROM_USECS_PER_DAY		86400000000L
#define STROM_DATE_NOBEGIN		(-2147483647 - 1)
#define STROM_DATE_NOEND		2147483647
#define STROM_TS_NOBEGIN		(-9223372036854775807L - 1)
#define STROM_TS_NOEND			9223372036854775807L
/*
 * Julian day 0 as a date: timestamp2tm (opencl_timelib.h:204-209) refuses a timestamp whose Julian
 * day is negative, and date(timestamp) / time(timestamp) turn that into CpuReCheck (246-250,
 * 271-275).  Its other bound, a Julian day above INT_MAX, cannot be reached: int64 microseconds
 * end near day 106751991.
 */
#define STROM_DATE_JULIAN_DAY0	(-2451545L)

#define STROM_TIME_COMPARE_FAMILY(pfx,TYPE)												\
	STROM_DEVICE pg_bool_t pgfn_##pfx##eq(cl_int *e, pg_##TYPE##_t a, pg_##TYPE##_t b)	\
	{ pg_bool_t r; r.isnull = a.isnull | b.isnull; r.value = (a.value == b.value); return r; }	\
	STROM_DEVICE pg_bool_t pgfn_##pfx##ne(cl_int *e, pg_##TYPE##_t a, pg_##TYPE##_t b)	\
	{ pg_bool_t r; r.isnull = a.isnull | b.isnull; r.value = (a.value != b.value); return r; }	\
	STROM_DEVICE pg_bool_t pgfn_##pfx##lt(cl_int *e, pg_##TYPE##_t a, pg_##TYPE##_t b)	\
	{ pg_bool_t r; r.isnull = a.isnull | b.isnull; r.value = (a.value <  b.value); return r; }	\
	STROM_DEVICE pg_bool_t pgfn_##pfx##le(cl_int *e, pg_##TYPE##_t a, pg_##TYPE##_t b)	\
	{ pg_bool_t r; r.isnull = a.isnull | b.isnull; r.value = (a.value <= b.value); return r; }	\
	STROM_DEVICE pg_bool_t pgfn_##pfx##gt(cl_int *e, pg_##TYPE##_t a, pg_##TYPE##_t b)	\
	{ pg_bool_t r; r.isnull = a.isnull | b.isnull; r.value = (a.value >  b.value); return r; }	\
	STROM_DEVICE pg_bool_t pgfn_##pfx##ge(cl_int *e, pg_##TYPE##_t a, pg_##TYPE##_t b)	\
	{ pg_bool_t r; r.isnull = a.isnull | b.isnull; r.value = (a.value >= b.value); return r; }	\
	STROM_DEVICE pg_int4_t pgfn_##pfx##cmp(cl_int *e, pg_##TYPE##_t a, pg_##TYPE##_t b)	\
	{ pg_int4_t r; r.isnull = a.isnull | b.isnull;										\
	  r.value = devfunc_int_comp(a.value, b.value); return r; }

STROM_TIME_COMPARE_FAMILY(date_, date)
STROM_TIME_COMPARE_FAMILY(time_, time)
STROM_TIME_COMPARE_FAMILY(timestamp_, timestamp)

/* date -> timestamp, +-infinity preserved, overflow -> CpuReCheck */
STROM_DEVICE pg_timestamp_t
pgfn_date_timestamp(cl_int *errcode, pg_date_t arg1)
{
	pg_timestamp_t result;
	result.isnull = arg1.isnull;
	result.value = 0;
	if (!result.isnull)
	{
		if (arg1.value == STROM_DATE_NOBEGIN)		result.value = STROM_TS_NOBEGIN;
		else if (arg1.value == STROM_DATE_NOEND)	result.value = STROM_TS_NOEND;
		else if (__builtin_mul_overflow((cl_long)arg1.value, STROM_USECS_PER_DAY, &result.value))
		{
			result.isnull = true;
			STROM_SET_ERROR(errcode, StromError_CpuReCheck);
		}
	}
	return result;
}

/* date(date), time(time), timestamp(timestamp): the catalog's alias casts (codegen.c:543-548, "ta/c:") */
STROM_DEVICE pg_date_t pgfn_date_date(cl_int *errcode, pg_date_t arg1) { return arg1; }
STROM_DEVICE pg_time_t pgfn_time_time(cl_int *errcode, pg_time_t arg1) { return arg1; }
STROM_DEVICE pg_timestamp_t pgfn_timestamp_timestamp(cl_int *errcode, pg_timestamp_t arg1) { return arg1; }

STROM_DEVICE pg_date_t
pgfn_timestamp_date(cl_int *errcode, pg_timestamp_t arg1)
{
	pg_date_t result;
	result.isnull = arg1.isnull;
	result.value = 0;
	if (!result.isnull)
	{
		if (arg1.value == STROM_TS_NOBEGIN)			result.value = STROM_DATE_NOBEGIN;
		else if (arg1.value == STROM_TS_NOEND)		result.value = STROM_DATE_NOEND;
		else
		{
			cl_long d = arg1.value / STROM_USECS_PER_DAY;
			if (arg1.value % STROM_USECS_PER_DAY < 0)
				d--;
			if (d < STROM_DATE_JULIAN_DAY0)
			{
				result.isnull = true;
				STROM_SET_ERROR(errcode, StromError_CpuReCheck);
			}
			else
				result.value = (cl_int)d;
		}
	}
	return result;
}

STROM_DEVICE pg_time_t
pgfn_timestamp_time(cl_int *errcode, pg_timestamp_t arg1)
{
	pg_time_t result;
	result.isnull = arg1.isnull;
	result.value = 0;
	if (!result.isnull)
	{
		if (arg1.value == STROM_TS_NOBEGIN || arg1.value == STROM_TS_NOEND)
			result.isnull = true;
		else
		{
			cl_long d = arg1.value / STROM_USECS_PER_DAY;
			cl_long t = arg1.value % STROM_USECS_PER_DAY;
			if (t < 0)
			{
				t += STROM_USECS_PER_DAY;
				d--;
			}
			if (d < STROM_DATE_JULIAN_DAY0)
			{
				result.isnull = true;
				STROM_SET_ERROR(errcode, StromError_CpuReCheck);
			}
			else
				result.value = t;
		}
	}
	return result;
}

/*
 * date +- integer: an infinite date stays what it is ("can't change infinity",
 * opencl_timelib.h:335, 353); a finite one is a checked add.  date - date with an infinite
 * operand goes back to the CPU (368).
 */
#define STROM_DATE_IS_INFINITE(d)	((d) == STROM_DATE_NOBEGIN || (d) == STROM_DATE_NOEND)

STROM_DEVICE pg_date_t
strom_date_add_days(cl_int *errcode, pg_date_t date, pg_int4_t days, bool subtract)
{
	pg_date_t result;
	result.isnull = date.isnull | days.isnull;
	result.value = 0;
	if (result.isnull)
		return result;
	if (STROM_DATE_IS_INFINITE(date.value))
		result.value = date.value;
	else if (subtract ? __builtin_sub_overflow(date.value, days.value, &result.value)
					  : __builtin_add_overflow(date.value, days.value, &result.value))
	{
		result.isnull = true;
		result.value = 0;
		STROM_SET_ERROR(errcode, StromError_CpuReCheck);
	}
	return result;
}
STROM_DEVICE pg_date_t
pgfn_date_pli(cl_int *errcode, pg_date_t arg1, pg_int4_t arg2)
{ return strom_date_add_days(errcode, arg1, arg2, false); }
STROM_DEVICE pg_date_t
pgfn_date_mii(cl_int *errcode, pg_date_t arg1, pg_int4_t arg2)
{ return strom_date_add_days(errcode, arg1, arg2, true); }
STROM_DEVICE pg_date_t
pgfn_integer_pl_date(cl_int *errcode, pg_int4_t arg1, pg_date_t arg2)
{ return strom_date_add_days(errcode, arg2, arg1, false); }

STROM_DEVICE pg_int4_t
pgfn_date_mi(cl_int *errcode, pg_date_t arg1, pg_date_t arg2)
{
	pg_int4_t result;
	result.isnull = arg1.isnull | arg2.isnull;
	result.value = 0;
	if (!result.isnull &&
		(STROM_DATE_IS_INFINITE(arg1.value) || STROM_DATE_IS_INFINITE(arg2.value) ||
		 __builtin_sub_overflow(arg1.value, arg2.value, &result.value)))
	{
		result.isnull = true;
		result.value = 0;
		STROM_SET_ERROR(errcode, StromError_CpuReCheck);
	}
	return result;
}

/*
 * The functions below promote their date through pgfn_date_timestamp, which may raise
 * CpuReCheck.  They are strict first: with the other argument NULL the date is not promoted,
 * so a NULL result never carries an error (strom_date_if).
 */
STROM_DEVICE pg_date_t
strom_date_if(pg_date_t date, bool other_isnull)
{
	date.isnull |= other_isnull;
	return date;
}

STROM_DEVICE pg_timestamp_t
pgfn_datetime_pl(cl_int *errcode, pg_date_t arg1, pg_time_t arg2)
{
	pg_timestamp_t result = pgfn_date_timestamp(errcode, strom_date_if(arg1, arg2.isnull));
	if (!result.isnull && result.value != STROM_TS_NOBEGIN && result.value != STROM_TS_NOEND &&
		__builtin_add_overflow(result.value, arg2.value, &result.value))
	{
		result.isnull = true;
		result.value = 0;
		STROM_SET_ERROR(errcode, StromError_CpuReCheck);
	}
	return result;
}
STROM_DEVICE pg_timestamp_t
pgfn_timedate_pl(cl_int *errcode, pg_time_t arg1, pg_date_t arg2)
{
	return pgfn_datetime_pl(errcode, arg2, arg1);
}

/* date <op> timestamp: promote the date, then compare */
#define STROM_DATE_TS_COMPARE(op,r_type)														\
	STROM_DEVICE pg_##r_type##_t																\
	pgfn_date_##op##_timestamp(cl_int *errcode, pg_date_t arg1, pg_timestamp_t arg2)			\
	{ return pgfn_timestamp_##op(errcode,														\
								 pgfn_date_timestamp(errcode, strom_date_if(arg1, arg2.isnull)), arg2); }	\
	STROM_DEVICE pg_##r_type##_t																\
	pgfn_timestamp_##op##_date(cl_int *errcode, pg_timestamp_t arg1, pg_date_t arg2)			\
	{ return pgfn_timestamp_##op(errcode, arg1,													\
								 pgfn_date_timestamp(errcode, strom_date_if(arg2, arg1.isnull))); }
STROM_DATE_TS_COMPARE(eq, bool)
STROM_DATE_TS_COMPARE(ne, bool)
STROM_DATE_TS_COMPARE(lt, bool)
STROM_DATE_TS_COMPARE(le, bool)
STROM_DATE_TS_COMPARE(gt, bool)
STROM_DATE_TS_COMPARE(ge, bool)
STROM_DATE_TS_COMPARE(cmp, int4)

#endif	/* STROM_TIMELIB_DEVICE_H */
